// 8-bit ingest of whole Deep360 frames: what the reference's loaders do on the host between the decoded PNGs and the
// two networks, on the frames as they decode -- (F, 12, H, W, 3) bytes, a frame's 12 panoramas in sorted file order.  See
// include/mode_hip.h.
//   mode_frames_u8_ingest  ToTensor + Normalize of every panorama (dataloader/preprocess.py:8, 64-69 on deep360_loader.py:108-109, 161-163)
//                          as a lookup in the host-built 256 x 3 table, and the split into left / right / fusion RGB
//   mode_rgb_half_pil      PIL.Image.resize((w / 2, h / 2)) of the four fusion panoramas (deep360_loader.py:151-153: Pillow's
//                          Resample.c, bicubic, 8 bits per channel: fixed point, horizontal pass, 8-bit store, vertical pass), then
//                          the same table
//   mode_decimate2         depth[::2, ::2] / conf[:, ::2, ::2] (deep360_loader.py:147-150) on the hand-off's planes
// All three are integer arithmetic, table lookups and copies: bit for bit what the host computes.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int kLut = 256 * 3;  // lut[v * 3 + c] = ((v / 255) - mean[c]) / std[c] as the host transform rounds it

__device__ __forceinline__ void load_lut(float* s_lut, const float* __restrict__ lut) {
  for (int i = threadIdx.x; i < kLut; i += NT) s_lut[i] = lut[i];
}

// ---------------------------------------------------------------------------------------------------------------------
// One thread per quad of pixels: 12 interleaved bytes in (three dwords), one float4 per colour plane out.  A panorama is
// 3 H W / 4 dwords, so quad q of the whole input starts at dword 3 q.
__global__ __launch_bounds__(NT) void frames_u8_ingest_kernel(const unsigned* __restrict__ frames, const float* __restrict__ lut,
                                                              long long quads, int quads_per_pano, float* __restrict__ left,
                                                              float* __restrict__ right, float* __restrict__ rgb) {
  __shared__ float s_lut[kLut];
  load_lut(s_lut, lut);
  __syncthreads();
  const long long hw = 4LL * quads_per_pano;
  for (long long q = (long long)blockIdx.x * NT + threadIdx.x; q < quads; q += (long long)gridDim.x * NT) {
    const unsigned w0 = frames[3 * q], w1 = frames[3 * q + 1], w2 = frames[3 * q + 2];
    const unsigned r[4] = {w0 & 255u, w0 >> 24, (w1 >> 16) & 255u, (w2 >> 8) & 255u};
    const unsigned g[4] = {(w0 >> 8) & 255u, w1 & 255u, w1 >> 24, (w2 >> 16) & 255u};
    const unsigned b[4] = {(w0 >> 16) & 255u, (w1 >> 8) & 255u, w2 & 255u, w2 >> 24};
    const float4 vr = make_float4(s_lut[3 * r[0]], s_lut[3 * r[1]], s_lut[3 * r[2]], s_lut[3 * r[3]]);
    const float4 vg = make_float4(s_lut[3 * g[0] + 1], s_lut[3 * g[1] + 1], s_lut[3 * g[2] + 1], s_lut[3 * g[3] + 1]);
    const float4 vb = make_float4(s_lut[3 * b[0] + 2], s_lut[3 * b[1] + 2], s_lut[3 * b[2] + 2], s_lut[3 * b[3] + 2]);
    const long long n = q / quads_per_pano;  // f * 12 + k
    const long long at = 4 * (q - n * quads_per_pano);
    const long long f = n / 12;
    const int k = (int)(n - 12 * f);
    float* d = ((k & 1) ? right : left) + (6 * f + (k >> 1)) * 3 * hw + at;  // pair k / 2 of frame f
    *reinterpret_cast<float4*>(d) = vr;
    *reinterpret_cast<float4*>(d + hw) = vg;
    *reinterpret_cast<float4*>(d + 2 * hw) = vb;
    if (rgb && (k < 2 || k >= 10)) {  // panoramas 0, 1, 10, 11 -> slots 0 .. 3 of the fusion RGB
      float* e = rgb + (12 * f + 3 * (k < 2 ? k : k - 8)) * hw + at;
      *reinterpret_cast<float4*>(e) = vr;
      *reinterpret_cast<float4*>(e + hw) = vg;
      *reinterpret_cast<float4*>(e + 2 * hw) = vb;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Pillow's two-pass 8-bit resize to half size, one launch: a block owns TH x TW output pixels of one panorama.  It stages the
// NR x NC input pixels its taps reach as whole dwords, runs the horizontal pass over all NR rows into LDS as bytes (Pillow stores that
// pass in 8 bits too), then the vertical pass out of LDS, the table lookup and the stores.  A table row is 10 ints: the first input
// index, the number of taps (<= 8) and 8 fixed-point coefficients.
constexpr int TH = 16, TW = 32;
constexpr int NR = 2 * TH + 6, NC = 2 * TW + 6;  // input rows / columns under a tile: 8 taps at stride 2
constexpr int ROWD = (NC * 3 + 3 + 3) / 4;       // dwords of a staged row: its bytes start up to 3 bytes into the first dword
constexpr int kTab = 10;
constexpr int kPrec = 22;  // Resample.c PRECISION_BITS = 32 - 8 - 2

__device__ __forceinline__ unsigned clip8(int acc) {
  const int v = acc >> kPrec;
  return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

__global__ __launch_bounds__(NT) void rgb_half_pil_kernel(const unsigned char* __restrict__ frames, const int* __restrict__ tab_w,
                                                          const int* __restrict__ tab_h, const float* __restrict__ lut, int H, int W,
                                                          int tiles_x, int tiles_y, float* __restrict__ rgb_half,
                                                          unsigned char* __restrict__ half_u8) {
  __shared__ float s_lut[kLut];
  __shared__ int s_tw[TW * kTab], s_th[TH * kTab];
  __shared__ unsigned s_in[NR * ROWD];
  __shared__ unsigned s_hq[NR * TW * 3 / 4];
  unsigned char* s_h = reinterpret_cast<unsigned char*>(s_hq);
  const unsigned char* s_inb = reinterpret_cast<const unsigned char*>(s_in);
  const int Ho = H / 2, Wo = W / 2;
  int bid = blockIdx.x;
  const int x0 = (bid % tiles_x) * TW;
  bid /= tiles_x;
  const int y0 = (bid % tiles_y) * TH;
  const int pz = bid / tiles_y;  // f * 4 + slot
  const int f = pz >> 2, slot = pz & 3;
  const int pano = 12 * f + (slot < 2 ? slot : slot + 8);
  const int tid = threadIdx.x;

  load_lut(s_lut, lut);
  for (int i = tid; i < TW * kTab; i += NT) s_tw[i] = x0 + i / kTab < Wo ? tab_w[(long long)x0 * kTab + i] : 0;
  for (int i = tid; i < TH * kTab; i += NT) s_th[i] = y0 + i / kTab < Ho ? tab_h[(long long)y0 * kTab + i] : 0;
  __syncthreads();

  // the input window of the tile; a table that points outside the image leaves an empty window (every tap below is bounds-checked)
  const int r_lo = s_th[0], c_lo = s_tw[0];
  const bool ok = r_lo >= 0 && r_lo < H && c_lo >= 0 && c_lo < W;
  const int nrows = ok ? min(NR, H - r_lo) : 0, ncols = ok ? min(NC, W - c_lo) : 0;
  const long long pano_b = (long long)pano * H * W * 3;  // a multiple of 4: H and W are even
  const unsigned* pano_d = reinterpret_cast<const unsigned*>(frames + pano_b);
  for (int i = tid; i < NR * ROWD; i += NT) {
    const int r = i / ROWD, d = i - r * ROWD;
    if (r < nrows) {
      const int b0 = ((r_lo + r) * W + c_lo) * 3;  // first byte of the row's window within the panorama (< 2^31: checked by the entry)
      const int d0 = b0 >> 2, d1 = (b0 + ncols * 3 + 3) >> 2;
      if (d0 + d < d1) s_in[i] = pano_d[d0 + d];
    }
  }
  __syncthreads();

  // horizontal pass: NR rows x TW output columns, three channels per thread
  for (int i = tid; i < NR * TW; i += NT) {
    const int r = i / TW, j = i - r * TW;
    if (r < nrows && x0 + j < Wo) {
      const int* t = s_tw + j * kTab;
      const int xmin = t[0] - c_lo, cnt = min(t[1], 8);
      const unsigned char* row = s_inb + r * (ROWD * 4) + ((((r_lo + r) * W + c_lo) * 3) & 3);
      int a0 = 1 << (kPrec - 1), a1 = a0, a2 = a0;
      for (int k = 0; k < cnt; ++k) {
        const int x = xmin + k;
        if (x >= 0 && x < ncols) {
          const int kk = t[2 + k];
          a0 += (int)row[3 * x] * kk;
          a1 += (int)row[3 * x + 1] * kk;
          a2 += (int)row[3 * x + 2] * kk;
        }
      }
      s_h[3 * i] = (unsigned char)clip8(a0);
      s_h[3 * i + 1] = (unsigned char)clip8(a1);
      s_h[3 * i + 2] = (unsigned char)clip8(a2);
    }
  }
  __syncthreads();

  // vertical pass: channel-major, so that a wave's fp32 stores are whole rows of a plane
  for (int i = tid; i < 3 * TH * TW; i += NT) {
    const int c = i / (TH * TW), rem = i - c * (TH * TW);
    const int yi = rem / TW, j = rem - yi * TW;
    const int y = y0 + yi, x = x0 + j;
    if (y < Ho && x < Wo) {
      const int* t = s_th + yi * kTab;
      const int ymin = t[0] - r_lo, cnt = min(t[1], 8);
      int acc = 1 << (kPrec - 1);
      for (int k = 0; k < cnt; ++k) {
        const int r = ymin + k;
        if (r >= 0 && r < nrows) acc += (int)s_h[(r * TW + j) * 3 + c] * t[2 + k];
      }
      const unsigned v = clip8(acc);
      const long long px = (long long)y * Wo + x;
      if (half_u8) half_u8[((long long)pz * Ho * Wo + px) * 3 + c] = (unsigned char)v;
      rgb_half[((long long)f * 12 + 3 * slot + c) * Ho * Wo + px] = s_lut[3 * v + c];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// out[n, y, x] = in[n, 2y, 2x].  kVec (W % 4 == 0, aligned buffers): a float4 in, a float2 out.
template <bool kVec>
__global__ __launch_bounds__(NT) void decimate2_kernel(const float* __restrict__ in, float* __restrict__ out, long long planes, int H,
                                                       int W) {
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const int per_row = kVec ? W / 4 : Wo;
  const long long total = planes * Ho * per_row;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
    const int x = (int)(i % per_row);
    const long long r = i / per_row;
    const int y = (int)(r % Ho);
    const long long n = r / Ho;
    const float* src = in + (n * H + 2 * y) * W;
    float* dst = out + (n * Ho + y) * Wo;
    if (kVec) {
      const float4 v = reinterpret_cast<const float4*>(src)[x];
      reinterpret_cast<float2*>(dst)[x] = make_float2(v.x, v.z);
    } else {
      dst[x] = src[2 * x];
    }
  }
}

// The adjoint of decimate2: gin[n, y, x] = gout[n, y / 2, x / 2] where y and x are both even, +0 elsewhere.  One thread per four
// consecutive elements of gin taken as one flat array (a quad may straddle rows and planes: any H and W); kVec (16-byte aligned gin):
// one 16-byte store per whole quad, single stores for the last, partial one.
template <bool kVec>
__global__ __launch_bounds__(NT) void decimate2_bwd_kernel(const float* __restrict__ gout, float* __restrict__ gin, long long total, int H,
                                                           int W) {
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const long long quads = (total + 3) / 4;
  for (long long q = (long long)blockIdx.x * NT + threadIdx.x; q < quads; q += (long long)gridDim.x * NT) {
    const long long i0 = 4 * q;
    long long row = i0 / W;  // n * H + y
    int x = (int)(i0 - row * W);
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int y = (int)(row % H);
      const long long n = row / H;
      v[e] = (i0 + e < total && !((x | y) & 1)) ? gout[(n * Ho + (y >> 1)) * Wo + (x >> 1)] : 0.f;
      if (++x == W) {
        x = 0;
        ++row;
      }
    }
    if (kVec && i0 + 4 <= total) {
      *reinterpret_cast<float4*>(gin + i0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (i0 + e < total) gin[i0 + e] = v[e];
    }
  }
}

int grid_for(long long n) { return (int)std::min<long long>(std::max<long long>((n + NT - 1) / NT, 1), 8LL * kNumCU); }

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// n * H * W * per < 2^31 without forming a product that could overflow (n >= 0, H, W, per > 0)
bool fits31(long long n, int H, int W, int per) {
  const long long lim = (1LL << 31) - 1, hw = (long long)H * W;
  return hw <= lim / per && n <= lim / per / hw;
}

}  // namespace

extern "C" int mode_frames_u8_ingest(const uint8_t* frames_u8, const float* lut, int F, int H, int W, float* left, float* right,
                                     float* rgb, mode_stream_t stream) {
  const char* who = "mode_frames_u8_ingest";
  MODE_REQUIRE(F >= 0 && H > 0 && W > 0, MODE_ERR_BAD_ARG, "%s: bad size %d x %d x %d", who, F, H, W);
  MODE_REQUIRE(fits31(F, H, W, 36), MODE_ERR_BAD_ARG, "%s: bad size %d x %d x %d (too large: 36 F H W >= 2^31)", who, F, H, W);
  MODE_REQUIRE(((long long)H * W) % 4 == 0, MODE_ERR_BAD_ARG, "%s: H W = %d x %d is not a multiple of 4", who, H, W);
  if (F == 0) return MODE_OK;
  MODE_REQUIRE(frames_u8 && lut && left && right, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  MODE_REQUIRE(aligned(frames_u8, 4), MODE_ERR_BAD_ARG, "%s: frames must be 4-byte aligned", who);
  MODE_REQUIRE(aligned(left, 16) && aligned(right, 16) && aligned(rgb, 16), MODE_ERR_BAD_ARG, "%s: outputs must be 16-byte aligned", who);
  const int qpp = (int)((long long)H * W / 4);
  const long long quads = 12LL * F * qpp;
  hipLaunchKernelGGL(frames_u8_ingest_kernel, dim3(grid_for(quads)), dim3(NT), 0, mode::as_stream(stream),
                     reinterpret_cast<const unsigned*>(frames_u8), lut, quads, qpp, left, right, rgb);
  return mode::check_launch(who);
}

extern "C" int mode_rgb_half_pil(const uint8_t* frames_u8, const int32_t* tab_w, const int32_t* tab_h, const float* lut, int F, int H,
                                 int W, float* rgb_half, uint8_t* half_u8, mode_stream_t stream) {
  const char* who = "mode_rgb_half_pil";
  MODE_REQUIRE(F >= 0 && H > 0 && W > 0, MODE_ERR_BAD_ARG, "%s: bad size %d x %d x %d", who, F, H, W);
  MODE_REQUIRE(fits31(F, H, W, 36), MODE_ERR_BAD_ARG, "%s: bad size %d x %d x %d (too large: 36 F H W >= 2^31)", who, F, H, W);
  MODE_REQUIRE(H % 2 == 0 && W % 2 == 0, MODE_ERR_BAD_ARG, "%s: %d x %d is not even (the tables are those of an exact halving)", who, H, W);
  if (F == 0) return MODE_OK;
  MODE_REQUIRE(frames_u8 && tab_w && tab_h && lut && rgb_half, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  MODE_REQUIRE(aligned(frames_u8, 4) && aligned(tab_w, 4) && aligned(tab_h, 4), MODE_ERR_BAD_ARG, "%s: frames and tables must be 4-byte aligned", who);
  const int tx = mode::cdiv(W / 2, TW), ty = mode::cdiv(H / 2, TH);
  const long long blocks = 4LL * F * tx * ty;  // < 2^31: at least one output pixel each
  hipLaunchKernelGGL(rgb_half_pil_kernel, dim3((unsigned)blocks), dim3(NT), 0, mode::as_stream(stream), frames_u8, tab_w, tab_h, lut, H, W,
                     tx, ty, rgb_half, half_u8);
  return mode::check_launch(who);
}

extern "C" int mode_decimate2(const float* in, float* out, long long planes, int H, int W, mode_stream_t stream) {
  const char* who = "mode_decimate2";
  MODE_REQUIRE(planes >= 0 && H > 0 && W > 0, MODE_ERR_BAD_ARG, "%s: bad size %lld x %d x %d", who, planes, H, W);
  MODE_REQUIRE(fits31(planes, H, W, 1), MODE_ERR_BAD_ARG, "%s: bad size %lld x %d x %d (too large)", who, planes, H, W);
  if (planes == 0) return MODE_OK;
  MODE_REQUIRE(in && out, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  MODE_REQUIRE(in != out, MODE_ERR_BAD_ARG, "%s: in-place operation is not possible", who);
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  hipStream_t st = mode::as_stream(stream);
  if (W % 4 == 0 && aligned(in, 16) && aligned(out, 8))
    hipLaunchKernelGGL(decimate2_kernel<true>, dim3(grid_for(planes * Ho * (W / 4))), dim3(NT), 0, st, in, out, planes, H, W);
  else
    hipLaunchKernelGGL(decimate2_kernel<false>, dim3(grid_for(planes * Ho * Wo)), dim3(NT), 0, st, in, out, planes, H, W);
  return mode::check_launch(who);
}

extern "C" int mode_decimate2_bwd(const float* gout, float* gin, long long planes, int H, int W, mode_stream_t stream) {
  const char* who = "mode_decimate2_bwd";
  MODE_REQUIRE(planes >= 0 && H > 0 && W > 0, MODE_ERR_BAD_ARG, "%s: bad size %lld x %d x %d", who, planes, H, W);
  MODE_REQUIRE(fits31(planes, H, W, 1), MODE_ERR_BAD_ARG, "%s: bad size %lld x %d x %d (too large)", who, planes, H, W);
  if (planes == 0) return MODE_OK;
  MODE_REQUIRE(gout && gin, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  MODE_REQUIRE(gout != gin, MODE_ERR_BAD_ARG, "%s: in-place operation is not possible", who);
  const long long total = planes * H * W;
  hipStream_t st = mode::as_stream(stream);
  if (aligned(gin, 16))
    hipLaunchKernelGGL(decimate2_bwd_kernel<true>, dim3(grid_for((total + 3) / 4)), dim3(NT), 0, st, gout, gin, total, H, W);
  else
    hipLaunchKernelGGL(decimate2_bwd_kernel<false>, dim3(grid_for((total + 3) / 4)), dim3(NT), 0, st, gout, gin, total, H, W);
  return mode::check_launch(who);
}
