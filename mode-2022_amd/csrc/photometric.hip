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
//
// The tile frame, the window arithmetic and the reduction are photometric_internal.h's, shared with the family's other losses; what
// is here is this loss's own: the 1-D warp and its staging, the smoothness on d / W, and the entries.
#include <type_traits>

#include "mode_hip_selfsup.h"
#include "photometric_internal.h"

namespace {

using namespace mode::photometric;

constexpr int kS = MODE_PHOTOMETRIC_STATS;
constexpr int kMaxK = MODE_PHOTOMETRIC_MAX_MAPS;

// Kernel-side copy of mode_photometric_params (by value: it travels in the kernel arguments).
struct Prm : Colour {
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
        pe += window_term(ssim, s.L[ch][i], s.R[ch][i], p.alpha);
      }
      acc[MODE_PHOTOMETRIC_N_VALID] += 1.0;
      acc[MODE_PHOTOMETRIC_SUM_PE] += (double)(pe * (1.f / 3.f));
    }
  }
  block_fold<kS, NT>(acc, sh, slab, [k](int j) { return (long long)k * kS + j; }, gridDim.x, col);
}

// One block: fold the columns of every (map, statistic) row in index order (thread t takes columns t, t + NT, ...; then the fixed
// butterfly and wave order), write stats (K x kS) and loss = sum_k wgt[k] (photo_k + lam smooth_k).
__global__ __launch_bounds__(NT) void photometric_final_kernel(const double* __restrict__ slab, int ncols, int K, int B, int H, int W, Prm p,
                                                               double* __restrict__ stats, float* __restrict__ loss) {
  __shared__ double sh[NT / 64][kMaxK * kS];
  __shared__ double fin[kMaxK * kS];
  fold_rows<kMaxK * kS, NT>(slab, ncols, K * kS, sh, stats, fin);
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
      win.tag[i] = wok[n] ? 1 : 0;
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

  const float scale = window_scale(p);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
#pragma unroll
    for (int n = 0; n < Windows::PER_THREAD; ++n) {
      const int i = threadIdx.x + n * NT;
      if (i < Windows::N) put_window<S::RW>(win, i, wok[n], s.L[ch], s.R[ch], scale, p);
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
        for (int dx = -1; dx <= 1; ++dx) a += window_share(win, wc + dy * Windows::RW + dx, x, y);
      if (win.tag[wc]) a += (1.f - p.alpha) * (1.f / 3.f) * sgn(y - x);
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

// The checks the two passes share; fills p and the tiling.
int check_common(const char* who, const float* left, const float* right, const float* disp, int view, int K, int B, int H, int W,
                 const mode_photometric_params* params, Prm& p, int& tiles_w, int& tiles) {
  MODE_REQUIRE(left && right && disp && params, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  MODE_REQUIRE(K >= 1 && K <= kMaxK, MODE_ERR_BAD_ARG, "%s: K = %d disparity maps (1 .. %d)", who, K, kMaxK);
  MODE_REQUIRE(B >= 1, MODE_ERR_BAD_ARG, "%s: bad batch size %d", who, B);
  int rc = check_tiling(who, H, W, tiles_w, tiles);
  if (rc != MODE_OK) return rc;
  // In-image offsets (3 H W), the workgroup index (B x tiles) and W as an exact float are 32-bit quantities; bases are 64-bit.
  MODE_REQUIRE(3ll * B * H * W < (1ll << 31) && W < (1 << 24), MODE_ERR_UNSUPPORTED,
               "%s: images of 3 x %d x %d x %d elements: 32-bit indices need 3 B H W < 2^31 (and W < 2^24)", who, B, H, W);
  load_colour(params, p);
  for (int k = 0; k < kMaxK; ++k) p.wgt[k] = k < K ? params->weights[k] : 0.f;
  MODE_REQUIRE(view == 0 || view == 1, MODE_ERR_BAD_ARG, "%s: view = %d (0: left, 1: right)", who, view);
  return MODE_OK;
}

// The (view, masked) form of the kernels, chosen once for both passes: f(view, masked) with the two as compile-time constants.
template <typename F>
void with_form(int view, bool masked, F f) {
  if (view == 0 && !masked) f(std::integral_constant<int, 0>(), std::false_type());
  if (view == 0 && masked) f(std::integral_constant<int, 0>(), std::true_type());
  if (view == 1 && !masked) f(std::integral_constant<int, 1>(), std::false_type());
  if (view == 1 && masked) f(std::integral_constant<int, 1>(), std::true_type());
}

// The forward of every entry of this file: two launches.  The entries of DESIGN 22 come with view 0 and no mask.
int view_loss_fwd(const char* who, const float* own_image, const float* other_image, const float* disp, const unsigned char* mask, int view,
                  int K, int B, int H, int W, const mode_photometric_params* params, void* workspace, size_t workspace_bytes, double* stats,
                  float* loss, mode_stream_t stream) {
  Prm p;
  int tiles_w, tiles;
  int rc = check_common(who, own_image, other_image, disp, view, K, B, H, W, params, p, tiles_w, tiles);
  if (rc != MODE_OK) return rc;
  MODE_REQUIRE(stats && loss, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  rc = check_workspace(who, workspace, workspace_bytes, mode_photometric_loss_workspace_bytes(K, B, H, W));
  if (rc != MODE_OK) return rc;
  double* slab = static_cast<double*>(workspace);
  hipStream_t st = mode::as_stream(stream);
  const int ncols = B * tiles;
  with_form(view, mask != nullptr, [&](auto v, auto m) {
    hipLaunchKernelGGL((photometric_fwd_kernel<decltype(v)::value, decltype(m)::value>), dim3(ncols, K), dim3(NT), 0, st, own_image,
                       other_image, disp, mask, B, H, W, tiles_w, tiles, p, slab);
  });
  hipLaunchKernelGGL(photometric_final_kernel, dim3(1), dim3(NT), 0, st, slab, ncols, K, B, H, W, p, stats, loss);
  return mode::check_launch(who);
}

// The backward: one launch.
int view_loss_bwd(const char* who, const float* own_image, const float* other_image, const float* disp, const unsigned char* mask, int view,
                  int K, int B, int H, int W, const mode_photometric_params* params, const double* stats, const float* gloss, float* gdisp,
                  mode_stream_t stream) {
  Prm p;
  int tiles_w, tiles;
  int rc = check_common(who, own_image, other_image, disp, view, K, B, H, W, params, p, tiles_w, tiles);
  if (rc != MODE_OK) return rc;
  MODE_REQUIRE(stats && gloss && gdisp, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  hipStream_t st = mode::as_stream(stream);
  with_form(view, mask != nullptr, [&](auto v, auto m) {
    hipLaunchKernelGGL((photometric_bwd_kernel<decltype(v)::value, decltype(m)::value>), dim3(B * tiles, K), dim3(NT), 0, st, own_image,
                       other_image, disp, mask, B, H, W, tiles_w, tiles, p, stats, gloss, gdisp);
  });
  return mode::check_launch(who);
}

}  // namespace

extern "C" size_t mode_photometric_loss_workspace_bytes(int K, int B, int H, int W) {
  if (K < 1 || K > kMaxK || B < 1 || H < 3 || W < 3 || 3ll * B * H * W >= (1ll << 31)) return 0;
  return ((size_t)K * kS * B * tiles_of(H, W) * sizeof(double) + 15) / 16 * 16;
}

extern "C" int mode_photometric_loss_fwd(const float* left, const float* right, const float* disp, int K, int B, int H, int W,
                                         const mode_photometric_params* params, void* workspace, size_t workspace_bytes, double* stats,
                                         float* loss, mode_stream_t stream) {
  return view_loss_fwd("mode_photometric_loss_fwd", left, right, disp, nullptr, 0, K, B, H, W, params, workspace, workspace_bytes, stats, loss,
                       stream);
}

extern "C" int mode_photometric_loss_bwd(const float* left, const float* right, const float* disp, int K, int B, int H, int W,
                                         const mode_photometric_params* params, const double* stats, const float* gloss, float* gdisp,
                                         mode_stream_t stream) {
  return view_loss_bwd("mode_photometric_loss_bwd", left, right, disp, nullptr, 0, K, B, H, W, params, stats, gloss, gdisp, stream);
}

// ---------------------------------------------------------------------------------------------- either view, with a mask
// include/mode_hip_selfsup.h.  The same kernels with the view and the mask as template parameters; view 0 without a mask launches the
// instantiation of the entries above.
extern "C" int mode_selfsup_view_loss_fwd(const float* own_image, const float* other_image, const float* disp, const unsigned char* mask,
                                          int view, int K, int B, int H, int W, const mode_photometric_params* params, void* workspace,
                                          size_t workspace_bytes, double* stats, float* loss, mode_stream_t stream) {
  return view_loss_fwd("mode_selfsup_view_loss_fwd", own_image, other_image, disp, mask, view, K, B, H, W, params, workspace, workspace_bytes,
                       stats, loss, stream);
}

extern "C" int mode_selfsup_view_loss_bwd(const float* own_image, const float* other_image, const float* disp, const unsigned char* mask,
                                          int view, int K, int B, int H, int W, const mode_photometric_params* params, const double* stats,
                                          const float* gloss, float* gdisp, mode_stream_t stream) {
  return view_loss_bwd("mode_selfsup_view_loss_bwd", own_image, other_image, disp, mask, view, K, B, H, W, params, stats, gloss, gdisp, stream);
}
