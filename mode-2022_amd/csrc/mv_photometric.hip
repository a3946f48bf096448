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
#include "mode_hip_mvvis.h"
#include "mv_photometric_internal.h"

namespace {

// grid = F * tiles.  Block col leaves its twelve statistics in column col of the slab and the winners of its tile in win.
// MASKED (include/mode_hip_mvvis.h): a pixel is valid for source s iff it is valid there and vis (F, S, H, W) != 0.
template <bool MASKED>
__global__ __launch_bounds__(NT) void mvphoto_fwd_kernel(const float* __restrict__ ref, const float* __restrict__ src,
                                                         const float* __restrict__ depth, Poses poses, int S, int H, int W, int tiles_w,
                                                         int tiles, Prm p, const unsigned char* __restrict__ vis,
                                                         unsigned char* __restrict__ win, double* __restrict__ slab) {
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
    if (MASKED) {  // a thread masks the validity bytes it has just written itself: no barrier in between
      const unsigned char* m = vis + HW * ((long long)f * S + sv);
#pragma unroll
      for (int k = 0; k < St::PER_THREAD; ++k) {
        const int i = threadIdx.x + k * NT;
        if (i >= St::N) continue;
        const int r = i / St::RW, c = i - r * St::RW;
        int h = (h0 - 1 + r) % H;
        h = h < 0 ? h + H : h;
        const int w = w0 - 1 + c;
        if (w >= 0 && w < W && s.ok[i] && !m[h * W + w]) s.ok[i] = 0;  // (columns outside [0, W) are invalid already)
      }
    }
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

// The forward entry and its masked form: the same checks, the same two launches.
template <bool MASKED>
int loss_fwd(const char* who, const float* ref, const float* src, const float* depth, const double* poses, int S, int F, int H, int W,
             const mode_photometric_params* params, void* workspace, size_t workspace_bytes, const unsigned char* vis, unsigned char* win,
             double* stats, float* loss, mode_stream_t stream) {
  Prm p;
  Poses ps;
  int tiles_w, tiles;
  MODE_REQUIRE(win && stats && loss && (vis || !MASKED), MODE_ERR_BAD_ARG, "%s: null pointer", who);
  int rc = check_common(who, ref, src, depth, poses, S, F, H, W, params, p, ps, tiles_w, tiles);
  if (rc != MODE_OK) return rc;
  rc = check_workspace(who, workspace, workspace_bytes, mode_mvphoto_workspace_bytes(S, F, H, W));
  if (rc != MODE_OK) return rc;
  double* slab = static_cast<double*>(workspace);
  hipStream_t st = mode::as_stream(stream);
  const int ncols = F * tiles;
  hipLaunchKernelGGL(mvphoto_fwd_kernel<MASKED>, dim3(ncols), dim3(NT), 0, st, ref, src, depth, ps, S, H, W, tiles_w, tiles, p, vis, win, slab);
  hipLaunchKernelGGL(mvphoto_final_kernel, dim3(1), dim3(NT), 0, st, slab, ncols, F, H, W, p, stats, loss);
  return mode::check_launch(who);
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
  return loss_fwd<false>("mode_mvphoto_loss_fwd", ref, src, depth, poses, S, F, H, W, params, workspace, workspace_bytes, nullptr, win, stats,
                         loss, stream);
}

extern "C" int mode_mvphoto_loss_fwd_masked(const float* ref, const float* src, const float* depth, const double* poses, int S, int F, int H,
                                            int W, const mode_photometric_params* params, void* workspace, size_t workspace_bytes,
                                            const unsigned char* vis, unsigned char* win, double* stats, float* loss, mode_stream_t stream) {
  return loss_fwd<true>("mode_mvphoto_loss_fwd_masked", ref, src, depth, poses, S, F, H, W, params, workspace, workspace_bytes, vis, win,
                        stats, loss, stream);
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
