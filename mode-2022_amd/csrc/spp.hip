// Spatial pyramid pooling block of the PSMNet extractor (ModeDisparity(conv='Regular'); reference models/submodule.py:228-268):
//   four AvgPool2d(k, stride k), k = 8, 16, 32, 64, of `skip`  ->  [1x1 conv + BatchNorm + ReLU per branch, elsewhere]  ->
//   four bilinear upsamplings (align_corners=True) back to (H, W) and the concatenation (raw, skip, k = 8, 16, 32, 64).
// NCHW fp32.  No atomics, every sum in a fixed order (bit-repeatable); every output element is written exactly once.
//
// Sizes (host-side refusals, in the style of size_contracts.h): offsets inside one plane are 32-bit, H * W < 2^30; plane offsets are
// 64-bit; the plane index is a grid dimension, N * C <= 65535 planes per launch (pooling: planes * tiles < 2^31 blocks).  Rows are
// moved 16 bytes per lane when W % 4 == 0 and every buffer is 16-byte aligned, one float per lane otherwise.
#include "common.h"

namespace {

constexpr int kLevels = 4;  // level l pools k = 8 << l

struct SppLevels {  // the four low-resolution tensors of one call: planes of h[l] x w[l]; sh / sw: the align_corners scales (in-1)/(out-1)
  float* p[kLevels];
  int h[kLevels], w[kLevels];
  float sh[kLevels], sw[kLevels];
};

// aten's area_pixel_compute_scale (align_corners): (in - 1) / (out - 1) in fp32, 0 for a single output
inline float ac_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

inline SppLevels make_levels(float* p8, float* p16, float* p32, float* p64, int H, int W) {
  SppLevels L;
  float* p[kLevels] = {p8, p16, p32, p64};
  for (int l = 0; l < kLevels; ++l) {
    L.p[l] = p[l];
    L.h[l] = H / (8 << l);
    L.w[l] = W / (8 << l);
    L.sh[l] = ac_scale(L.h[l], H);
    L.sw[l] = ac_scale(L.w[l], W);
  }
  return L;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---------------------------------------------------------------------------------------------------------------- pooling, forward
// One workgroup reduces a 64 x 64 region of one plane: a thread sums 4 rows x 4 columns, then 8 x 8 blocks of k = 8, 4 x 4 of k = 16,
// 2 x 2 of k = 32 and the one of k = 64 through LDS, each level from the sums of the level below (block j of 2k = blocks 2j, 2j+1 of k).
// Rows / columns beyond the k = 8 crop (floor(H / 8) * 8) are never read; a block of level k is written only inside floor(H / k) x
// floor(W / k) -- such a block consists of valid blocks of the level below, so the zeros standing for the uncovered part never reach it.
template <int V>
__global__ __launch_bounds__(256) void spp_pool_fwd_kernel(const float* __restrict__ x, SppLevels o, int H, int W, int tiles_w, int tiles) {
  __shared__ float s4[16][17];
  __shared__ float s8[8][8];
  __shared__ float s16[4][4];
  __shared__ float s32[2][2];
  const int t = threadIdx.x;
  const long long plane = blockIdx.x / tiles;
  const int tile = blockIdx.x % tiles, ty = tile / tiles_w, tx = tile % tiles_w;
  const int c4 = t & 15, rg = t >> 4;
  const int row0 = ty * 64 + rg * 4, col0 = tx * 64 + c4 * 4;
  float s = 0.f;
  if (row0 < o.h[0] * 8 && col0 < o.w[0] * 8) {  // (the crop is a multiple of 8: the 4 x 4 patch is inside or outside as a whole)
    const float* p = x + plane * H * W + (long long)row0 * W + col0;
    float r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (V == 4) {
        const float4 v = *reinterpret_cast<const float4*>(p + (long long)i * W);
        r[i] = (v.x + v.y) + (v.z + v.w);
      } else {
        const float* q = p + (long long)i * W;
        r[i] = (q[0] + q[1]) + (q[2] + q[3]);
      }
    }
    s = (r[0] + r[1]) + (r[2] + r[3]);
  }
  s4[rg][c4] = s;
  __syncthreads();
  if (t < 64) {
    const int by = t >> 3, bx = t & 7;
    const float v = (s4[2 * by][2 * bx] + s4[2 * by][2 * bx + 1]) + (s4[2 * by + 1][2 * bx] + s4[2 * by + 1][2 * bx + 1]);
    s8[by][bx] = v;
    const int gy = ty * 8 + by, gx = tx * 8 + bx;
    if (gy < o.h[0] && gx < o.w[0]) o.p[0][(plane * o.h[0] + gy) * o.w[0] + gx] = v * (1.f / 64.f);
  }
  __syncthreads();
  if (t < 16) {
    const int by = t >> 2, bx = t & 3;
    const float v = (s8[2 * by][2 * bx] + s8[2 * by][2 * bx + 1]) + (s8[2 * by + 1][2 * bx] + s8[2 * by + 1][2 * bx + 1]);
    s16[by][bx] = v;
    const int gy = ty * 4 + by, gx = tx * 4 + bx;
    if (gy < o.h[1] && gx < o.w[1]) o.p[1][(plane * o.h[1] + gy) * o.w[1] + gx] = v * (1.f / 256.f);
  }
  __syncthreads();
  if (t < 4) {
    const int by = t >> 1, bx = t & 1;
    const float v = (s16[2 * by][2 * bx] + s16[2 * by][2 * bx + 1]) + (s16[2 * by + 1][2 * bx] + s16[2 * by + 1][2 * bx + 1]);
    s32[by][bx] = v;
    const int gy = ty * 2 + by, gx = tx * 2 + bx;
    if (gy < o.h[2] && gx < o.w[2]) o.p[2][(plane * o.h[2] + gy) * o.w[2] + gx] = v * (1.f / 1024.f);
  }
  __syncthreads();
  if (t == 0 && ty < o.h[3] && tx < o.w[3])
    o.p[3][(plane * o.h[3] + ty) * o.w[3] + tx] = ((s32[0][0] + s32[0][1]) + (s32[1][0] + s32[1][1])) * (1.f / 4096.f);
}

// --------------------------------------------------------------------------------------------------------------- pooling, backward
// gskip[n, c, h, w] = gcat[n, c0 + c, h, w] + sum over the levels of g_k[n, c, h / k, w / k] / k^2 where (h, w) lies inside the level's
// crop: slice + (((k = 64) + 32) + 16) + 8), the order in which autograd meets them too.  One pass; the slice is read where it lies
// (gcat == nullptr: no slice term).
template <int V>
__global__ __launch_bounds__(256) void spp_pool_bwd_kernel(const float* __restrict__ gcat, int C, int c0, SppLevels g, float* __restrict__ gskip,
                                                           int Cs, int H, int W) {
  const int WV = W / V;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= H * WV) return;
  const int h = q / WV, w0 = (q - h * WV) * V;
  const int nc = blockIdx.y, n = nc / Cs, c = nc - n * Cs;
  const long long HW = (long long)H * W;
  const int at = h * W + w0;
  float v[V];
  if (gcat) {
    const float* src = gcat + ((long long)n * C + c0 + c) * HW + at;
    if constexpr (V == 4) {
      const float4 a = *reinterpret_cast<const float4*>(src);
      v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
    } else {
      v[0] = src[0];
    }
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = 0.f;
  }
  float p = 0.f;  // the pyramid's part, coarsest level first: the small terms meet before the large ones
#pragma unroll
  for (int l = kLevels - 1; l >= 0; --l) {
    const int sh = 3 + l;  // k = 8 << l
    const float inv = 1.f / (float)(1 << (2 * sh));
    // (V == 4: w0 is a multiple of 4 and the crop a multiple of 8, so the four columns share their block)
    if ((h >> sh) < g.h[l] && (w0 >> sh) < g.w[l]) p += g.p[l][((long long)nc * g.h[l] + (h >> sh)) * g.w[l] + (w0 >> sh)] * inv;
  }
#pragma unroll
  for (int j = 0; j < V; ++j) v[j] += p;
  float* dst = gskip + (long long)nc * HW + at;
  if constexpr (V == 4)
    *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
  else
    dst[0] = v[0];
}

// ------------------------------------------------------------------------------------------------- upsampling + concatenation, forward
// aten's upsample_bilinear2d with align_corners=True: src = scale * dst, i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1
// (a 1-pixel source axis: scale 0, i0 = i1 = 0, l0 = 1 -- it broadcasts).
struct Tap {
  int i0, i1;
  float l0, l1;
};
__device__ __forceinline__ Tap tap_of(float scale, int dst, int in) {
  Tap t;
  const float src = scale * (float)dst;
  t.i0 = min((int)src, in - 1);
  t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
  t.l1 = src - (float)t.i0;
  t.l0 = 1.f - t.l1;
  return t;
}

// One thread writes V consecutive pixels of one row of one output plane: blockIdx.y = n * C + c, channels in the reference's order
// raw (Cr), skip (Cs), then Cb channels of each level k = 8, 16, 32, 64.
template <int V>
__global__ __launch_bounds__(256) void spp_concat_fwd_kernel(const float* __restrict__ raw, const float* __restrict__ skip, SppLevels b,
                                                             float* __restrict__ out, int Cr, int Cs, int Cb, int H, int W) {
  const int WV = W / V;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= H * WV) return;
  const int h = q / WV, w0 = (q - h * WV) * V;
  const int C = Cr + Cs + kLevels * Cb;
  const int nc = blockIdx.y, n = nc / C, c = nc - n * C;
  const long long HW = (long long)H * W;
  const int at = h * W + w0;
  float v[V];
  if (c < Cr + Cs) {
    const float* src = (c < Cr ? raw + ((long long)n * Cr + c) * HW : skip + ((long long)n * Cs + (c - Cr)) * HW) + at;
    if constexpr (V == 4) {
      const float4 a = *reinterpret_cast<const float4*>(src);
      v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
    } else {
      v[0] = src[0];
    }
  } else {
    const int l = (c - Cr - Cs) / Cb, cb = (c - Cr - Cs) - l * Cb;
    const int hk = b.h[l], wk = b.w[l];
    const float* src = b.p[l] + ((long long)n * Cb + cb) * hk * wk;
    const Tap th = tap_of(b.sh[l], h, hk);
    const float* r0 = src + th.i0 * wk;
    const float* r1 = src + th.i1 * wk;
    const float sw = b.sw[l];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const Tap tw = tap_of(sw, w0 + j, wk);
      v[j] = th.l0 * (tw.l0 * r0[tw.i0] + tw.l1 * r0[tw.i1]) + th.l1 * (tw.l0 * r1[tw.i0] + tw.l1 * r1[tw.i1]);
    }
  }
  float* dst = out + (long long)nc * HW + at;
  if constexpr (V == 4)
    *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
  else
    dst[0] = v[0];
}

// ------------------------------------------------------------------------------------------------ upsampling + concatenation, backward
// graw = the first Cr channels of every sample of gcat, contiguous.
template <int V>
__global__ __launch_bounds__(256) void spp_slice_copy_kernel(const float* __restrict__ gcat, float* __restrict__ graw, int C, int Cr, int HWV) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= HWV) return;
  const int nc = blockIdx.y, n = nc / Cr, c = nc - n * Cr;
  const long long HW = (long long)HWV * V;
  const float* src = gcat + ((long long)n * C + c) * HW + (long long)q * V;
  float* dst = graw + (long long)nc * HW + (long long)q * V;
  if constexpr (V == 4)
    *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(src);
  else
    dst[0] = src[0];
}

// The destination indices whose taps touch source index y: a contiguous range, since i0 grows with the destination.  Bracketed from
// y - 1 <= scale * dst < y + 1 with a margin, then tightened with the forward's own arithmetic.
__device__ __forceinline__ bool touches(float scale, int dst, int in, int y) {
  const Tap t = tap_of(scale, dst, in);
  return t.i0 == y || t.i1 == y;
}
__device__ __forceinline__ void support_of(float scale, int in, int out, int y, int& lo, int& hi) {
  lo = 0, hi = out - 1;
  if (in > 1 && scale > 0.f) {
    const float inv = 1.f / scale;
    lo = max(0, (int)floorf((float)(y - 1) * inv) - 1);
    hi = min(out - 1, (int)ceilf((float)(y + 1) * inv) + 1);
  }
  while (lo < hi && !touches(scale, lo, in, y)) ++lo;
  while (hi > lo && !touches(scale, hi, in, y)) --hi;
}
__device__ __forceinline__ float weight_of(float scale, int dst, int in, int y) {
  const Tap t = tap_of(scale, dst, in);
  return (t.i0 == y ? t.l0 : 0.f) + (t.i1 == y ? t.l1 : 0.f);  // (the last source index: i0 == i1, both taps)
}

// Adjoint of the upsampling of one level, in gather form: T threads (one wave, or the workgroup of four) own one low-resolution pixel
// (n, cb, y, x) and sum wy(h) * wx(w) * g[h, w] over its support -- thread i the terms i, i + T, ... in ascending order (row-major
// over the support), then a butterfly over the wave's lanes and, for T = 256, ((w0 + w1) + (w2 + w3)) over the four waves.
template <int T>
__global__ __launch_bounds__(256) void spp_up_adjoint_kernel(const float* __restrict__ gcat, float* __restrict__ gb, int C, int c0, int Cb, int hk,
                                                             int wk, float sh, float sw, int H, int W, long long n_out) {
  __shared__ float part[4];
  const long long o = (long long)blockIdx.x * (256 / T) + threadIdx.x / T;
  const int lane = threadIdx.x % T;
  if (T == 64 && o >= n_out) return;  // (wave-uniform; the T = 256 grid has exactly n_out blocks)
  const int x = (int)(o % wk), y = (int)((o / wk) % hk);
  const long long ncb = o / ((long long)wk * hk);
  const int cb = (int)(ncb % Cb), n = (int)(ncb / Cb);
  const float* g = gcat + ((long long)n * C + c0 + cb) * H * W;
  int h_lo, h_hi, w_lo, w_hi;
  support_of(sh, hk, H, y, h_lo, h_hi);
  support_of(sw, wk, W, x, w_lo, w_hi);
  const int ncol = w_hi - w_lo + 1, terms = (h_hi - h_lo + 1) * ncol;
  float acc = 0.f;
  for (int i = lane; i < terms; i += T) {
    const int r = i / ncol, h = h_lo + r, w = w_lo + (i - r * ncol);
    if (touches(sh, h, hk, y) && touches(sw, w, wk, x)) acc += (weight_of(sh, h, hk, y) * weight_of(sw, w, wk, x)) * g[h * W + w];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (T == 64) {
    if (lane == 0) gb[o] = acc;
  } else {
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) gb[o] = (part[0] + part[1]) + (part[2] + part[3]);
  }
}

int check_plane(const char* who, int H, int W) {
  MODE_REQUIRE(H > 0 && W > 0, MODE_ERR_BAD_ARG, "%s: non-positive plane size %d x %d", who, H, W);
  MODE_REQUIRE(H >= 64 && W >= 64, MODE_ERR_UNSUPPORTED, "%s: the k = 64 level needs planes of at least 64 x 64 (got %d x %d)", who, H, W);
  MODE_REQUIRE((long long)H * W < (1ll << 30), MODE_ERR_UNSUPPORTED, "%s: plane of %d x %d is beyond 2^30 elements", who, H, W);
  return MODE_OK;
}

}  // namespace

extern "C" int mode_spp_pool_fwd(const float* x, float* y8, float* y16, float* y32, float* y64, long long planes, int H, int W,
                                 mode_stream_t stream) {
  MODE_REQUIRE(planes >= 0, MODE_ERR_BAD_ARG, "mode_spp_pool_fwd: negative plane count");
  if (int rc = check_plane("mode_spp_pool_fwd", H, W)) return rc;
  if (planes == 0) return MODE_OK;
  MODE_REQUIRE(x && y8 && y16 && y32 && y64, MODE_ERR_BAD_ARG, "mode_spp_pool_fwd: null pointer");
  const SppLevels o = make_levels(y8, y16, y32, y64, H, W);
  const int tiles_h = mode::cdiv(o.h[0] * 8, 64), tiles_w = mode::cdiv(o.w[0] * 8, 64), tiles = tiles_h * tiles_w;
  MODE_REQUIRE(planes * tiles < (1ll << 31), MODE_ERR_UNSUPPORTED, "mode_spp_pool_fwd: %lld planes x %d tiles is beyond 2^31 workgroups", planes, tiles);
  const dim3 grid((unsigned)(planes * tiles));
  if (W % 4 == 0 && aligned16(x))
    spp_pool_fwd_kernel<4><<<grid, 256, 0, mode::as_stream(stream)>>>(x, o, H, W, tiles_w, tiles);
  else
    spp_pool_fwd_kernel<1><<<grid, 256, 0, mode::as_stream(stream)>>>(x, o, H, W, tiles_w, tiles);
  return mode::check_launch("mode_spp_pool_fwd");
}

extern "C" int mode_spp_pool_bwd(const float* gcat, int C, int c0, const float* g8, const float* g16, const float* g32, const float* g64,
                                 float* gskip, int N, int Cs, int H, int W, mode_stream_t stream) {
  MODE_REQUIRE(N >= 0 && Cs > 0, MODE_ERR_BAD_ARG, "mode_spp_pool_bwd: bad sizes N %d Cs %d", N, Cs);
  if (int rc = check_plane("mode_spp_pool_bwd", H, W)) return rc;
  MODE_REQUIRE(!gcat || (c0 >= 0 && C >= c0 + Cs), MODE_ERR_BAD_ARG, "mode_spp_pool_bwd: channels %d .. %d outside the %d of gcat", c0, c0 + Cs, C);
  if (N == 0) return MODE_OK;
  MODE_REQUIRE(g8 && g16 && g32 && g64 && gskip, MODE_ERR_BAD_ARG, "mode_spp_pool_bwd: null pointer");
  MODE_REQUIRE((long long)N * Cs <= 65535, MODE_ERR_UNSUPPORTED, "mode_spp_pool_bwd: %lld planes (> 65535)", (long long)N * Cs);
  const SppLevels g = make_levels(const_cast<float*>(g8), const_cast<float*>(g16), const_cast<float*>(g32), const_cast<float*>(g64), H, W);
  const bool vec = W % 4 == 0 && aligned16(gcat) && aligned16(gskip);
  const dim3 grid(mode::cdiv((long long)H * (W / (vec ? 4 : 1)), 256), N * Cs);
  if (vec)
    spp_pool_bwd_kernel<4><<<grid, 256, 0, mode::as_stream(stream)>>>(gcat, C, c0, g, gskip, Cs, H, W);
  else
    spp_pool_bwd_kernel<1><<<grid, 256, 0, mode::as_stream(stream)>>>(gcat, C, c0, g, gskip, Cs, H, W);
  return mode::check_launch("mode_spp_pool_bwd");
}

extern "C" int mode_spp_concat_fwd(const float* raw, const float* skip, const float* b8, const float* b16, const float* b32, const float* b64,
                                   float* out, int N, int Cr, int Cs, int Cb, int H, int W, mode_stream_t stream) {
  MODE_REQUIRE(N >= 0 && Cr > 0 && Cs > 0 && Cb > 0, MODE_ERR_BAD_ARG, "mode_spp_concat_fwd: bad sizes N %d Cr %d Cs %d Cb %d", N, Cr, Cs, Cb);
  if (int rc = check_plane("mode_spp_concat_fwd", H, W)) return rc;
  if (N == 0) return MODE_OK;
  MODE_REQUIRE(raw && skip && b8 && b16 && b32 && b64 && out, MODE_ERR_BAD_ARG, "mode_spp_concat_fwd: null pointer");
  const long long planes = (long long)N * (Cr + Cs + (long long)kLevels * Cb);
  MODE_REQUIRE(planes <= 65535, MODE_ERR_UNSUPPORTED, "mode_spp_concat_fwd: %lld planes (> 65535)", planes);
  const SppLevels b = make_levels(const_cast<float*>(b8), const_cast<float*>(b16), const_cast<float*>(b32), const_cast<float*>(b64), H, W);
  const bool vec = W % 4 == 0 && aligned16(raw) && aligned16(skip) && aligned16(out);
  const dim3 grid(mode::cdiv((long long)H * (W / (vec ? 4 : 1)), 256), (unsigned)planes);
  if (vec)
    spp_concat_fwd_kernel<4><<<grid, 256, 0, mode::as_stream(stream)>>>(raw, skip, b, out, Cr, Cs, Cb, H, W);
  else
    spp_concat_fwd_kernel<1><<<grid, 256, 0, mode::as_stream(stream)>>>(raw, skip, b, out, Cr, Cs, Cb, H, W);
  return mode::check_launch("mode_spp_concat_fwd");
}

extern "C" int mode_spp_concat_bwd(const float* gcat, float* graw, float* gb8, float* gb16, float* gb32, float* gb64, int N, int Cr, int Cs,
                                   int Cb, int H, int W, mode_stream_t stream) {
  MODE_REQUIRE(N >= 0 && Cr > 0 && Cs > 0 && Cb > 0, MODE_ERR_BAD_ARG, "mode_spp_concat_bwd: bad sizes N %d Cr %d Cs %d Cb %d", N, Cr, Cs, Cb);
  if (int rc = check_plane("mode_spp_concat_bwd", H, W)) return rc;
  if (N == 0) return MODE_OK;
  MODE_REQUIRE(gcat && graw && gb8 && gb16 && gb32 && gb64, MODE_ERR_BAD_ARG, "mode_spp_concat_bwd: null pointer");
  const int C = Cr + Cs + kLevels * Cb;
  MODE_REQUIRE((long long)N * C <= 65535, MODE_ERR_UNSUPPORTED, "mode_spp_concat_bwd: %lld planes (> 65535)", (long long)N * C);
  MODE_REQUIRE((long long)N * Cb * (H / 8) * (W / 8) < (1ll << 31), MODE_ERR_UNSUPPORTED, "mode_spp_concat_bwd: branch gradient beyond 2^31 elements");
  const hipStream_t st = mode::as_stream(stream);
  const bool vec = W % 4 == 0 && aligned16(gcat) && aligned16(graw);
  const int HWV = H * W / (vec ? 4 : 1);
  const dim3 cgrid(mode::cdiv(HWV, 256), N * Cr);
  if (vec)
    spp_slice_copy_kernel<4><<<cgrid, 256, 0, st>>>(gcat, graw, C, Cr, HWV);
  else
    spp_slice_copy_kernel<1><<<cgrid, 256, 0, st>>>(gcat, graw, C, Cr, HWV);
  if (int rc = mode::check_launch("mode_spp_concat_bwd (raw)")) return rc;
  const SppLevels b = make_levels(gb8, gb16, gb32, gb64, H, W);
  for (int l = 0; l < kLevels; ++l) {
    const int hk = b.h[l], wk = b.w[l];
    const long long n_out = (long long)N * Cb * hk * wk;
    // terms per low-resolution pixel: about two source intervals each way (the whole axis for a 1-pixel source)
    const long long rows = hk > 1 ? std::min<long long>(H, 2ll * (H - 1) / (hk - 1) + 3) : H;
    const long long cols = wk > 1 ? std::min<long long>(W, 2ll * (W - 1) / (wk - 1) + 3) : W;
    const int c0 = Cr + Cs + l * Cb;
    if (rows * cols > 2048)  // the workgroup per pixel (k = 32, 64 at the full size: 6 700 and 22 000 terms)
      spp_up_adjoint_kernel<256><<<dim3((unsigned)n_out), 256, 0, st>>>(gcat, b.p[l], C, c0, Cb, hk, wk, b.sh[l], b.sw[l], H, W, n_out);
    else
      spp_up_adjoint_kernel<64><<<dim3((unsigned)((n_out + 3) / 4)), 256, 0, st>>>(gcat, b.p[l], C, c0, Cb, hk, wk, b.sh[l], b.sw[l], H, W, n_out);
    if (int rc = mode::check_launch("mode_spp_concat_bwd (adjoint)")) return rc;
  }
  return MODE_OK;
}
