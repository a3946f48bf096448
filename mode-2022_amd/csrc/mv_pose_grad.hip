// The gradient of the multi-view reprojection loss with respect to the sources' poses (include/mode_hip_mvpose.h has the
// definition): the reduction, over every pixel-source pair, of the chain  loss -> window minima -> Ih_s -> (u, v) -> Y = D (A n) + o
// -> [A | o].
//
// The frame is mvphoto_bwd_kernel's, from the same pieces (mv_photometric_internal.h, photometric_internal.h): one workgroup per
// 16 x 32 tile of one frame, the tile and a halo of two staged once for every source, the winners of the tile and its ring, the source
// loop inside.  For a source that won a window here, Ih_s is staged with the bilinear's two partial slopes per channel of the tile's
// own pixels (two LDS planes where the backward has one, because the pose moves u and v independently); the window coefficients are
// formed channel by channel exactly as the backward forms them, and a pixel sums G_u = sum_c a_c Ih_u,c and G_v = sum_c a_c Ih_v,c
// in registers and leaves both in LDS.  Then the thread that holds the depth and the viewing direction of a tile pixel (the staging
// assignment, which is not the window assignment) rebuilds Y, rho^2 and Y_y^2 + Y_z^2 in fp64 -- one sqrt and two divisions, no
// transcendental --, forms g_Y = G_u grad_Y u + G_v grad_Y v and adds its twelve products with (D n, 1) to twelve fp64 sums.  The
// Jacobians exist only there, after the channel loop.
//
// The reduction is the scheme of photometric_internal.h: a thread walks its pixels in ascending order, a fixed butterfly, the waves
// in index order, slab column (source, statistic; workgroup), and a second launch of one block per source folds the columns in index
// order and scales by gloss / max(N, 1).  A source without a window in a tile gets zeros in that column, so every column the fold
// reads was written.  No atomics; the same inputs give the same bits on any stream.
#include "mode_hip_mvpose.h"
#include "mv_photometric_internal.h"

namespace {

constexpr int kG = 12;  // the entries of one source's 3 x 4 table

// stage_src<2, true> with the two partial slopes kept apart: d Ih / du and d Ih / dv of the tile's own pixels into
// su[ch][r * TW + c], sv[ch][r * TW + c] (0 where the pixel is invalid for the source).  The expressions are sample<true>'s.
__device__ __forceinline__ void stage_src_uv(Stage<2>& s, const float* __restrict__ img, const double* __restrict__ P, int H, int W,
                                             const Prm& p, const Dir (&n)[Stage<2>::PER_THREAD], const float (&dep)[Stage<2>::PER_THREAD],
                                             float (*su)[TH * TW], float (*sv)[TH * TW]) {
  using S = Stage<2>;
  const int HW = H * W;
#pragma unroll
  for (int k = 0; k < S::PER_THREAD; ++k) {
    const int i = threadIdx.x + k * NT;
    if (i >= S::N) continue;
    Geo g;
    float ih[3] = {0.f, 0.f, 0.f}, iu[3] = {0.f, 0.f, 0.f}, iv[3] = {0.f, 0.f, 0.f};
    const bool ok = project<false>(dep[k], n[k], P, H, W, g);
    if (ok) {
      const int a = g.ya * W + g.x0, b = g.yb * W + g.x0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float* pl = img + c * HW;
        const float r00 = pl[a] * p.std[c] + p.mean[c], r01 = pl[a + 1] * p.std[c] + p.mean[c];
        const float r10 = pl[b] * p.std[c] + p.mean[c], r11 = pl[b + 1] * p.std[c] + p.mean[c];
        const float top = (1.f - g.t) * r00 + g.t * r01, bot = (1.f - g.t) * r10 + g.t * r11;
        ih[c] = (1.f - g.q) * top + g.q * bot;
        iu[c] = (1.f - g.q) * (r01 - r00) + g.q * (r11 - r10);
        iv[c] = bot - top;
      }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) s.R[ch][i] = ih[ch];
    s.ok[i] = ok ? 1 : 0;
    const int r = i / S::RW - 2, c = i % S::RW - 2;
    if (r >= 0 && r < TH && c >= 0 && c < TW) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        su[ch][r * TW + c] = iu[ch];
        sv[ch][r * TW + c] = iv[ch];
      }
    }
  }
}

// grid = F * tiles.  Block col leaves, for every source sv, its twelve sums in column col of slab rows 12 sv .. 12 sv + 11.
__global__ __launch_bounds__(NT) void mvpose_grad_kernel(const float* __restrict__ ref, const float* __restrict__ src,
                                                         const float* __restrict__ depth, Poses poses, int S, int H, int W, int tiles_w,
                                                         int tiles, Prm p, const unsigned char* __restrict__ win,
                                                         double* __restrict__ slab) {
  using St = Stage<2>;
  __shared__ St s;
  __shared__ Windows wn;
  __shared__ float su[3][TH * TW], sv_[3][TH * TW];
  __shared__ float Gu[TH * TW], Gv[TH * TW];
  __shared__ double sh[NT / 64][kG];
  const int col = blockIdx.x;
  const int ncols = gridDim.x;
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

  const float scale = window_scale(p);
  for (int sv = 0; sv < S; ++sv) {
    int any = 0;
#pragma unroll
    for (int k = 0; k < Windows::PER_THREAD; ++k) any |= mine[k] == sv;
    if (!__syncthreads_or(any)) {  // (the barrier: the previous source's planes have been read.)  No window here is s's
      if (threadIdx.x < kG) slab[((long long)sv * kG + threadIdx.x) * ncols + col] = 0.0;
      continue;
    }
    stage_src_uv(s, src + 3 * HW * ((long long)f * S + sv), poses.p[sv], H, W, p, n, dep, su, sv_);
    __syncthreads();
    float gu[PX], gv[PX];
#pragma unroll
    for (int k = 0; k < PX; ++k) gu[k] = gv[k] = 0.f;
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
        gu[k] += su[ch][j] * a;  // (the slopes are 0 where the pixel is invalid for s; no window of s contains such a pixel)
        gv[k] += sv_[ch][j] * a;
      }
      __syncthreads();  // the next channel overwrites the windows
    }
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      Gu[threadIdx.x + k * NT] = gu[k];
      Gv[threadIdx.x + k * NT] = gv[k];
    }
    __syncthreads();

    // The staging assignment: this thread has D and n of staged pixel i in registers.  Tile rows at and beyond H are other tiles'
    // pixels (rows wrap), tile columns at and beyond W are invalid for every source.
    double acc[kG];
#pragma unroll
    for (int j = 0; j < kG; ++j) acc[j] = 0.0;
    const double* __restrict__ P = poses.p[sv];
#pragma unroll
    for (int k = 0; k < St::PER_THREAD; ++k) {
      const int i = threadIdx.x + k * NT;
      if (i >= St::N) continue;
      const int r = i / St::RW - 2, c = i % St::RW - 2;
      if (r < 0 || r >= TH || c < 0 || c >= TW || h0 + r >= H || !s.ok[i]) continue;
      const float fu = Gu[r * TW + c], fv = Gv[r * TW + c];
      const double D = (double)dep[k];
      const double Xx = D * n[k].x, Xy = D * n[k].y, Xz = D * n[k].z;  // the point in the reference's axes
      const double Yx = P[0] * Xx + P[1] * Xy + P[2] * Xz + P[3];
      const double Yy = P[4] * Xx + P[5] * Xy + P[6] * Xz + P[7];
      const double Yz = P[8] * Xx + P[9] * Xy + P[10] * Xz + P[11];
      const double s2 = Yy * Yy + Yz * Yz;
      const double r2 = Yx * Yx + s2;
      const double ku = -((double)W / kPi) * (double)fu / (r2 * sqrt(s2));  // G_u grad_Y u = ku (e_x rho^2 - Y_x Y)
      const double kv = -((double)H / (2.0 * kPi)) * (double)fv / s2;       // G_v grad_Y v = kv (0, Y_z, -Y_y)
      const double gx = ku * s2;                                            // (rho^2 - Y_x^2 = Y_y^2 + Y_z^2)
      const double gy = -ku * Yx * Yy + kv * Yz;
      const double gz = -ku * Yx * Yz - kv * Yy;
      acc[0] += gx * Xx;
      acc[1] += gx * Xy;
      acc[2] += gx * Xz;
      acc[3] += gx;
      acc[4] += gy * Xx;
      acc[5] += gy * Xy;
      acc[6] += gy * Xz;
      acc[7] += gy;
      acc[8] += gz * Xx;
      acc[9] += gz * Xy;
      acc[10] += gz * Xz;
      acc[11] += gz;
    }
    block_fold<kG, NT>(acc, sh, slab, [sv](int j) { return (long long)sv * kG + j; }, ncols, col);
  }
}

// One block per source: fold the columns of its twelve sums in index order and scale by gloss / max(N, 1).
__global__ __launch_bounds__(NT) void mvpose_final_kernel(const double* __restrict__ slab, int ncols, const double* __restrict__ stats,
                                                          const float* __restrict__ gloss, double* __restrict__ gposes) {
  __shared__ double sh[NT / 64][kG];
  __shared__ double raw[kG], fin[kG];
  const int sv = blockIdx.x;
  fold_rows<kG, NT>(slab + (long long)sv * kG * ncols, ncols, kG, sh, raw, fin);
  __syncthreads();
  if (threadIdx.x < kG) {
    const double n_valid = stats[MODE_MVP_N];
    gposes[sv * kG + threadIdx.x] = fin[threadIdx.x] * ((double)gloss[0] / (n_valid > 1.0 ? n_valid : 1.0));
  }
}

}  // namespace

extern "C" int mode_mvpose_version(void) { return MODE_MVPOSE_VERSION; }

extern "C" size_t mode_mvpose_workspace_bytes(int S, int F, int H, int W) {
  if (S < 1 || S > kMaxS || F < 1 || H < 3 || W < 3 || 3ll * F * S * H * W >= (1ll << 31)) return 0;
  return ((size_t)kG * S * F * tiles_of(H, W) * sizeof(double) + 15) / 16 * 16;
}

extern "C" int mode_mvpose_grad(const float* ref, const float* src, const float* depth, const double* poses, int S, int F, int H, int W,
                                const mode_photometric_params* params, const unsigned char* win, const double* stats, const float* gloss,
                                void* workspace, size_t workspace_bytes, double* gposes, mode_stream_t stream) {
  const char* who = "mode_mvpose_grad";
  Prm p;
  Poses ps;
  int tiles_w, tiles;
  MODE_REQUIRE(win && stats && gloss && gposes, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  int rc = check_common(who, ref, src, depth, poses, S, F, H, W, params, p, ps, tiles_w, tiles);
  if (rc != MODE_OK) return rc;
  rc = check_workspace(who, workspace, workspace_bytes, mode_mvpose_workspace_bytes(S, F, H, W));
  if (rc != MODE_OK) return rc;
  double* slab = static_cast<double*>(workspace);
  hipStream_t st = mode::as_stream(stream);
  const int ncols = F * tiles;
  hipLaunchKernelGGL(mvpose_grad_kernel, dim3(ncols), dim3(NT), 0, st, ref, src, depth, ps, S, H, W, tiles_w, tiles, p, win, slab);
  hipLaunchKernelGGL(mvpose_final_kernel, dim3(S), dim3(NT), 0, st, slab, ncols, stats, gloss, gposes);
  return mode::check_launch(who);
}
