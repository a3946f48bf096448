// Left-right consistency of a stereo pair's two disparity maps, with the occlusion masks it yields (DESIGN 24;
// include/mode_hip_selfsup.h has the definition).  A view is (s, own, other): left = (-1, dl, dr), right = (+1, dr, dl); a pixel of a
// view samples the other map at x = w + s own along its own row and is charged |own - other(x)|.
//
// The term has no coupling along H: one workgroup per row of one (map, batch element).  The row of both maps is staged in LDS once
// and both views are built from it.  The forward writes the two mask bytes of every pixel and leaves six statistics per workgroup in
// its slab column (the two folds of photometric_internal.h: a thread walks its pixels in ascending order, a fixed butterfly, the
// waves in index order, a one-block fold of the columns in index order; fp32 terms, fp64 sums).
//
// The gradient into the SAMPLED map is a scatter by nature.  Here it is a gather: 0 <= own <= dmax is part of validity, so the source
// columns that can reach target column c lie in c - 1 <= w <= c + 1 + dmax (left view) or c - 1 - dmax <= w <= c + 1 (right view).  Every
// pixel leaves a record (x0 and the sign of own - oh in one word; t in another) in LDS, and a thread per target walks its window in
// ascending w and adds in that order.  No atomics; every output element is written exactly once; the arithmetic of a pixel does not
// depend on where its row lies, so rolling the inputs along H rolls the masks and the gradients bit for bit.
#include "mode_hip_selfsup.h"
#include "photometric_internal.h"

static_assert(MODE_LR_MAX_MAPS == MODE_PHOTOMETRIC_MAX_MAPS, "mode_hip_selfsup.h restates MODE_PHOTOMETRIC_MAX_MAPS as a literal");
static_assert(MODE_SELFSUP_VIEW_STATS == MODE_PHOTOMETRIC_STATS, "mode_hip_selfsup.h restates MODE_PHOTOMETRIC_STATS as a literal");

namespace {

using namespace mode::photometric;  // NT threads per workgroup; sgn; the two folds; the workspace check

constexpr int kS = MODE_LR_STATS;
constexpr int kMaxK = MODE_LR_MAX_MAPS;
constexpr int kAcc = 2 * kS;            // both views' statistics of one row
constexpr int kRows = 2 * kMaxK * kS;   // slab rows: (view, map, statistic)
constexpr int kNoRecord = -4;           // the record of a pixel that sends nothing: below 2 c - 2 for every column c >= 0
constexpr int NTF = 1024;               // threads of the fold: one block, and the more loads in flight the sooner it is done

struct Prm {
  float tau, dmax;
  float wgt[kMaxK];
};

// One pixel of one view.  own, other: the staged rows; sf = (float)s.  e = own - oh (signed), o0 / o1 the two samples.
struct Pixel {
  bool valid;
  int x0;
  float t, diff, o0, o1;
};

__device__ __forceinline__ Pixel lr_pixel(const float* __restrict__ own, const float* __restrict__ other, int W, int w, float sf, float dmax) {
  Pixel p;
  const float d = own[w];
  const float x = (float)w + sf * d;
  p.valid = __builtin_isfinite(d) && d >= 0.f && d <= dmax && x >= 0.f && x <= (float)(W - 1);
  p.x0 = 0;
  p.t = p.diff = p.o0 = p.o1 = 0.f;
  if (p.valid) {
    int x0 = (int)floorf(x);
    x0 = x0 < W - 2 ? x0 : W - 2;
    const float o0 = other[x0], o1 = other[x0 + 1];
    if (__builtin_isfinite(o0) && __builtin_isfinite(o1)) {
      p.x0 = x0;
      p.t = x - (float)x0;
      p.o0 = o0;
      p.o1 = o1;
      p.diff = d - ((1.f - p.t) * o0 + p.t * o1);
    } else {
      p.valid = false;
    }
  }
  return p;
}

__device__ __forceinline__ void stage_rows(float* __restrict__ rl, float* __restrict__ rr, const float* __restrict__ gl,
                                           const float* __restrict__ gr, int W) {
  for (int w = threadIdx.x; w < W; w += NT) {
    rl[w] = gl[w];
    rr[w] = gr[w];
  }
}

// grid = (B * H, K); dynamic LDS: 2 W floats.  Block (col, k) leaves its six statistics in column col of the slab rows of map k.
__global__ __launch_bounds__(NT) void lr_fwd_kernel(const float* __restrict__ dl, const float* __restrict__ dr, int K, int B, int H, int W,
                                                    Prm p, unsigned char* __restrict__ mask, double* __restrict__ slab) {
  extern __shared__ float lds[];
  __shared__ double sh[NT / 64][kAcc];
  float* rl = lds;
  float* rr = lds + W;
  const int col = blockIdx.x, k = blockIdx.y;
  const long long row = ((long long)k * B * H + col) * W;  // (k, b, h) rows are contiguous: col = b * H + h
  stage_rows(rl, rr, dl + row, dr + row, W);
  __syncthreads();
  const long long view_stride = (long long)K * B * H * W;
  double acc[kAcc] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int w = threadIdx.x; w < W; w += NT) {
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const Pixel q = v == 0 ? lr_pixel(rl, rr, W, w, -1.f, p.dmax) : lr_pixel(rr, rl, W, w, 1.f, p.dmax);
      const float e = fabsf(q.diff);
      const bool vis = q.valid && e <= p.tau;
      if (q.valid) {
        acc[v * kS + MODE_LR_N_VALID] += 1.0;
        acc[v * kS + MODE_LR_SUM_E] += (double)e;
      }
      if (vis) acc[v * kS + MODE_LR_N_VISIBLE] += 1.0;
      if (mask) mask[v * view_stride + row + w] = vis ? 1 : 0;
    }
  }
  block_fold<kAcc, NT>(acc, sh, slab, [K, k](int a) {  // accumulator a = (view, statistic) -> slab row (view, map, statistic)
    const int v = a / kS, j = a - v * kS;
    return ((long long)v * K + k) * kS + j;
  }, gridDim.x, col);
}

// One block: fold the columns of every (view, map, statistic) row in index order; write stats (2, K, kS) and
// loss = sum_k wgt[k] (lr_left_k + lr_right_k).
__global__ __launch_bounds__(NTF) void lr_final_kernel(const double* __restrict__ slab, int ncols, int K, Prm p, double* __restrict__ stats,
                                                      float* __restrict__ loss) {
  __shared__ double sh[NTF / 64][kRows];
  __shared__ double fin[kRows];
  fold_rows<kRows, NTF>(slab, ncols, 2 * K * kS, sh, stats, fin);
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = 0.0;
    for (int k = 0; k < K; ++k) {
      double term = 0.0;
      for (int view = 0; view < 2; ++view) {
        const double* f = fin + (view * K + k) * kS;
        const double n = f[MODE_LR_N_VALID];
        term += f[MODE_LR_SUM_E] / (n > 1.0 ? n : 1.0);
      }
      total += (double)p.wgt[k] * term;
    }
    loss[0] = (float)total;
  }
}

// What the sources of one view send to target column c: the records of columns lo .. hi (clamped to the row) in ascending order.
// rx: (x0 << 1) | (own < oh), or kNoRecord; rt: t.  cf = gloss wgt / N of that view.
__device__ __forceinline__ float take(float a, int r, const float* __restrict__ rt, int w, int first, float cf) {
  const unsigned u = (unsigned)(r - first);  // one subtraction and one comparison per record: most records end here
  if (u < 4u) {
    const float t = rt[w];
    const float sn = (u & 1u) ? cf : -cf;  // -sign(own - oh) / N
    a += sn * (u < 2u ? t : 1.f - t);      // x0 + 1 == c takes t, x0 == c takes 1 - t
  }
  return a;
}

__device__ __forceinline__ float gather(const int* __restrict__ rx, const float* __restrict__ rt, int lo, int hi, int c, float cf) {
  constexpr int U = 8;  // records fetched ahead of their tests: one LDS round trip per U records instead of one each
  float a = 0.f;
  const int first = 2 * c - 2;  // the four records that reach c: x0 == c - 1 (words 2c - 2, 2c - 1) and x0 == c (2c, 2c + 1)
  int w = lo;
  for (; w + U - 1 <= hi; w += U) {
    int r[U];
#pragma unroll
    for (int j = 0; j < U; ++j) r[j] = rx[w + j];
#pragma unroll
    for (int j = 0; j < U; ++j) a = take(a, r[j], rt, w + j, first, cf);
  }
  for (; w <= hi; ++w) a = take(a, rx[w], rt, w, first, cf);
  return a;
}

// grid = (B * H, K); dynamic LDS: 2 W floats (the rows) + 2 views x W x (int + float) (the records).
__global__ __launch_bounds__(NT) void lr_bwd_kernel(const float* __restrict__ dl, const float* __restrict__ dr, int K, int B, int H, int W,
                                                    Prm p, int reach, const double* __restrict__ stats, const float* __restrict__ gloss,
                                                    float* __restrict__ gdl, float* __restrict__ gdr) {
  extern __shared__ float lds[];
  float* rl = lds;
  float* rr = lds + W;
  int* rx = reinterpret_cast<int*>(lds + 2 * W);  // [2][W]
  float* rt = lds + 4 * W;                        // [2][W]
  const int col = blockIdx.x, k = blockIdx.y;
  const long long row = ((long long)k * B * H + col) * W;
  stage_rows(rl, rr, dl + row, dr + row, W);
  __syncthreads();
  float cf[2];
#pragma unroll
  for (int v = 0; v < 2; ++v) {
    const double n = stats[(v * K + k) * kS + MODE_LR_N_VALID];
    cf[v] = (float)((double)gloss[0] * (double)p.wgt[k] / (n > 1.0 ? n : 1.0));
  }
  for (int w = threadIdx.x; w < W; w += NT) {
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const Pixel q = v == 0 ? lr_pixel(rl, rr, W, w, -1.f, p.dmax) : lr_pixel(rr, rl, W, w, 1.f, p.dmax);
      const bool sends = q.valid && q.diff != 0.f;
      rx[v * W + w] = sends ? (q.x0 << 1) | (q.diff < 0.f ? 1 : 0) : kNoRecord;
      rt[v * W + w] = q.t;
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < W; c += NT) {
    // dl: its own (left) view's direct part, then what the right view's pixels sampled from it (sources c - 1 - dmax .. c + 1)
    const Pixel ql = lr_pixel(rl, rr, W, c, -1.f, p.dmax);
    float g = ql.valid ? sgn(ql.diff) * (1.f + (ql.o1 - ql.o0)) * cf[0] : 0.f;
    int lo = c - 1 - reach, hi = c + 1;
    g += gather(rx + W, rt + W, lo > 0 ? lo : 0, hi < W - 1 ? hi : W - 1, c, cf[1]);
    gdl[row + c] = g;
    // dr: the right view's direct part, then the left view's samples (sources c - 1 .. c + 1 + dmax)
    const Pixel qr = lr_pixel(rr, rl, W, c, 1.f, p.dmax);
    g = qr.valid ? sgn(qr.diff) * (1.f - (qr.o1 - qr.o0)) * cf[1] : 0.f;
    lo = c - 1;
    hi = c + 1 + reach;
    g += gather(rx, rt, lo > 0 ? lo : 0, hi < W - 1 ? hi : W - 1, c, cf[0]);
    gdr[row + c] = g;
  }
}

int check_common(const char* who, const float* dl, const float* dr, int K, int B, int H, int W, const mode_lr_params* params, Prm& p) {
  MODE_REQUIRE(dl && dr && params, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  MODE_REQUIRE(K >= 1 && K <= kMaxK, MODE_ERR_BAD_ARG, "%s: K = %d disparity maps (1 .. %d)", who, K, kMaxK);
  MODE_REQUIRE(B >= 1 && H >= 1, MODE_ERR_BAD_ARG, "%s: bad batch size %d or height %d", who, B, H);
  MODE_REQUIRE(W >= 2, MODE_ERR_BAD_ARG, "%s: W = %d: W must be at least 2 (two samples of the other map)", who, W);
  MODE_REQUIRE(__builtin_isfinite(params->tau) && params->tau > 0.f, MODE_ERR_BAD_ARG, "%s: tau = %g must be finite and positive", who, (double)params->tau);
  MODE_REQUIRE(__builtin_isfinite(params->dmax) && params->dmax > 0.f, MODE_ERR_BAD_ARG, "%s: dmax = %g must be finite and positive", who,
               (double)params->dmax);
  MODE_REQUIRE((long long)B * H < (1ll << 31), MODE_ERR_UNSUPPORTED, "%s: %d x %d rows: one workgroup per row needs B H < 2^31", who, B, H);
  MODE_REQUIRE(W <= MODE_LR_MAX_W, MODE_ERR_UNSUPPORTED, "%s: W = %d: the row staging holds W <= %d", who, W, MODE_LR_MAX_W);
  MODE_REQUIRE(params->dmax <= (float)W, MODE_ERR_UNSUPPORTED, "%s: dmax = %g is beyond W = %d", who, (double)params->dmax, W);
  p.tau = params->tau;
  p.dmax = params->dmax;
  for (int k = 0; k < kMaxK; ++k) p.wgt[k] = k < K ? params->weights[k] : 0.f;
  return MODE_OK;
}

}  // namespace

extern "C" int mode_selfsup_version(void) { return MODE_SELFSUP_VERSION; }

extern "C" size_t mode_lr_consistency_workspace_bytes(int K, int B, int H, int W) {
  if (K < 1 || K > kMaxK || B < 1 || H < 1 || W < 2 || W > MODE_LR_MAX_W || (long long)B * H >= (1ll << 31)) return 0;
  return ((size_t)2 * K * kS * B * H * sizeof(double) + 15) / 16 * 16;
}

extern "C" int mode_lr_consistency_fwd(const float* disp_l, const float* disp_r, int K, int B, int H, int W, const mode_lr_params* params,
                                       void* workspace, size_t workspace_bytes, unsigned char* mask, double* stats, float* loss,
                                       mode_stream_t stream) {
  const char* who = "mode_lr_consistency_fwd";
  Prm p;
  int rc = check_common(who, disp_l, disp_r, K, B, H, W, params, p);
  if (rc != MODE_OK) return rc;
  MODE_REQUIRE(stats && loss, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  rc = check_workspace(who, workspace, workspace_bytes, mode_lr_consistency_workspace_bytes(K, B, H, W));
  if (rc != MODE_OK) return rc;
  double* slab = static_cast<double*>(workspace);
  hipStream_t st = mode::as_stream(stream);
  const int ncols = B * H;
  hipLaunchKernelGGL(lr_fwd_kernel, dim3(ncols, K), dim3(NT), 2 * (size_t)W * sizeof(float), st, disp_l, disp_r, K, B, H, W, p, mask, slab);
  hipLaunchKernelGGL(lr_final_kernel, dim3(1), dim3(NTF), 0, st, slab, ncols, K, p, stats, loss);
  return mode::check_launch(who);
}

extern "C" int mode_lr_consistency_bwd(const float* disp_l, const float* disp_r, int K, int B, int H, int W, const mode_lr_params* params,
                                       const double* stats, const float* gloss, float* gdisp_l, float* gdisp_r, mode_stream_t stream) {
  const char* who = "mode_lr_consistency_bwd";
  Prm p;
  int rc = check_common(who, disp_l, disp_r, K, B, H, W, params, p);
  if (rc != MODE_OK) return rc;
  MODE_REQUIRE(stats && gloss && gdisp_l && gdisp_r, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  const int reach = (int)ceilf(p.dmax);  // <= W: checked
  hipLaunchKernelGGL(lr_bwd_kernel, dim3(B * H, K), dim3(NT), 6 * (size_t)W * sizeof(float), mode::as_stream(stream), disp_l, disp_r, K, B, H,
                     W, p, reach, stats, gloss, gdisp_l, gdisp_r);
  return mode::check_launch(who);
}
