// Stereo pairs at any working size: what the reference's Deep360DatasetDisparity does on the host when a pair is stored at
// another width than the working one (dataloader/deep360_loader.py:92-106) -- PIL.Image.resize((w, h)) of both panoramas, cv2.resize(...,
// INTER_NEAREST) * (w / stored_w) of the disparity map, the training crop -- on the decoded bytes.  See include/mode_hip.h.
//   mode_images_u8_resize_pil   Pillow's Resample.c for 8-bit images and the default bicubic filter between any two sizes (up to 4 x per
//                               axis either way): the horizontal pass, its result stored in 8 bits, the vertical pass; a pass whose size
//                               does not change is skipped.  One launch per pass that runs, a thread per output pixel of the pass, a
//                               plain loop over the taps the host-built table names.  Bytes are read and written one at a time: a row of
//                               37 x 3 bytes is no multiple of 4 and nothing here assumes it were.
//   mode_disp_resize_nearest    src[rows[y], cols[x]] * ratio, one fp32 multiply
// Both take an optional per-image window of the resized image and compute nothing outside it (of the horizontal pass: only the source
// rows the window's vertical taps reach).  Integer arithmetic, table lookups and one multiply: bit for bit what the host computes.
// The tables and the windows live in device memory.  Their values are clamped where they form an address (a tap outside the source is
// dropped, a window is moved inside the image, a nearest index is clamped), so no value of theirs can move an access outside a buffer.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int kLut = 256 * 3;                       // lut[v * 3 + c]: see ingest.hip
constexpr int kPrec = 22;                           // Resample.c PRECISION_BITS = 32 - 8 - 2
constexpr int kMaxScale = 4;                        // per axis, either way (MODE_RESIZE_MAX_SCALE)
constexpr int kMaxTaps = 2 * (2 * kMaxScale) + 1;   // ksize = 2 ceil(2 max(scale, 1)) + 1 at scale 4

__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> kPrec;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// One axis' table: row i = [first source index, number of taps, ksize coefficients]; n = the source's size along the axis.
struct Tab {
  const int* t;
  int stride;  // 2 + ksize
  int n;
};

// The taps of output index i that lie inside the source: source indices [first, last); the coefficient of source index s is kk[s - lo].
struct Taps {
  const int* kk;
  int lo, first, last;
};

__device__ __forceinline__ Taps taps_of(const Tab& tab, int i) {
  const int* row = tab.t + i * tab.stride;
  const int cnt = min(max(row[1], 0), tab.stride - 2);
  Taps r;
  r.kk = row + 2;
  r.lo = min(max(row[0], -kMaxTaps), tab.n);  // (a first index outside [-cnt, n) leaves no tap either way; this keeps lo + cnt in range)
  r.first = max(r.lo, 0);
  r.last = min(max(r.lo + cnt, r.first), tab.n);  // s - lo in [0, cnt) for every s in [first, last): inside the row
  return r;
}

struct Geom {
  int N, Hs, Ws, H, W, h_win, w_win, per, split;
};

// (top, left) of image n's window, moved inside the (H, W) image whatever the table holds
__device__ __forceinline__ int2 window_of(const int* __restrict__ windows, const Geom& g, int n) {
  int top = 0, left = 0;
  if (windows) {
    top = windows[2 * (n / g.per)];
    left = windows[2 * (n / g.per) + 1];
  }
  return make_int2(min(max(top, 0), g.H - g.h_win), min(max(left, 0), g.W - g.w_win));
}

struct Out {
  unsigned char* u8;  // (N, h_win, w_win, 3) or null
  float* f32;         // (N, 3, h_win, w_win) or null
};

// pixel (y, x) of image n's window: the bytes, and / or their normalised values as planes
__device__ __forceinline__ void emit(const Out& o, const Geom& g, const float* s_lut, int n, int y, int x, int v0, int v1, int v2) {
  const int slot = g.split ? (n % g.per) * (g.N / g.per) + n / g.per : n;
  const int hw = g.h_win * g.w_win, px = y * g.w_win + x;
  if (o.u8) {
    unsigned char* d = o.u8 + (slot * hw + px) * 3;
    d[0] = (unsigned char)v0, d[1] = (unsigned char)v1, d[2] = (unsigned char)v2;
  }
  if (o.f32) {
    float* d = o.f32 + slot * 3 * hw + px;
    d[0] = s_lut[3 * v0], d[hw] = s_lut[3 * v1 + 1], d[2 * hw] = s_lut[3 * v2 + 2];
  }
}

__device__ __forceinline__ void load_lut(float* s_lut, const float* __restrict__ lut, bool wanted) {
  if (wanted)
    for (int i = threadIdx.x; i < kLut; i += NT) s_lut[i] = lut[i];
  __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------------------
// The horizontal pass.  grid = (ceil(R w_win / NT), min(N, 65535)), R = the rows the pass covers.
//   kFinal (the height does not change): rows top .. top + h_win of the source, straight to the outputs.
//   otherwise: every source row that the window's vertical taps reach, columns left .. left + w_win, as bytes into
//   mid (N, Hs, w_win, 3); the other rows of mid are neither written here nor read by the vertical pass.
template <bool kFinal>
__global__ __launch_bounds__(NT) void resize_h_kernel(const unsigned char* __restrict__ src, Tab tw, Tab th, const int* __restrict__ windows,
                                                      Geom g, const float* __restrict__ lut, Out o, unsigned char* __restrict__ mid) {
  __shared__ float s_lut[kLut];
  load_lut(s_lut, lut, kFinal && o.f32);
  const int R = kFinal ? g.h_win : g.Hs;
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= R * g.w_win) return;
  const int y = i / g.w_win, x = i - y * g.w_win;
  for (int n = blockIdx.y; n < g.N; n += gridDim.y) {
    const int2 win = window_of(windows, g, n);
    int r = y;
    if (kFinal) {
      r = win.x + y;
    } else {
      const int r_lo = taps_of(th, win.x).first, r_hi = taps_of(th, win.x + g.h_win - 1).last;
      if (r < r_lo || r >= r_hi) continue;
    }
    const Taps t = taps_of(tw, win.y + x);
    const unsigned char* row = src + (n * g.Hs + r) * g.Ws * 3;
    int a0 = 1 << (kPrec - 1), a1 = a0, a2 = a0;
    for (int s = t.first; s < t.last; ++s) {
      const int kk = t.kk[s - t.lo];
      a0 += (int)row[3 * s] * kk;
      a1 += (int)row[3 * s + 1] * kk;
      a2 += (int)row[3 * s + 2] * kk;
    }
    if (kFinal) {
      emit(o, g, s_lut, n, y, x, clip8(a0), clip8(a1), clip8(a2));
    } else {
      unsigned char* d = mid + ((n * g.Hs + r) * g.w_win + x) * 3;
      d[0] = (unsigned char)clip8(a0), d[1] = (unsigned char)clip8(a1), d[2] = (unsigned char)clip8(a2);
    }
  }
}

// The vertical pass over src (N, Hs, ws, 3): mid (ws = w_win, col0 = 0) after a horizontal pass, or the images themselves (ws = Ws = W,
// col0 = the window's left) when the width does not change.  grid = (ceil(h_win w_win / NT), min(N, 65535)).
template <bool kFromMid>
__global__ __launch_bounds__(NT) void resize_v_kernel(const unsigned char* __restrict__ src, Tab th, const int* __restrict__ windows, Geom g,
                                                      const float* __restrict__ lut, Out o) {
  __shared__ float s_lut[kLut];
  load_lut(s_lut, lut, o.f32 != nullptr);
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= g.h_win * g.w_win) return;
  const int y = i / g.w_win, x = i - y * g.w_win;
  const int ws = kFromMid ? g.w_win : g.Ws;
  for (int n = blockIdx.y; n < g.N; n += gridDim.y) {
    const int2 win = window_of(windows, g, n);
    const Taps t = taps_of(th, win.x + y);
    const unsigned char* col = src + (n * g.Hs * ws + (kFromMid ? 0 : win.y) + x) * 3;
    int a0 = 1 << (kPrec - 1), a1 = a0, a2 = a0;
    for (int s = t.first; s < t.last; ++s) {
      const int kk = t.kk[s - t.lo];
      const unsigned char* p = col + s * ws * 3;
      a0 += (int)p[0] * kk;
      a1 += (int)p[1] * kk;
      a2 += (int)p[2] * kk;
    }
    emit(o, g, s_lut, n, y, x, clip8(a0), clip8(a1), clip8(a2));
  }
}

// Neither size changes: the window of the source, as bytes and / or normalised planes.
__global__ __launch_bounds__(NT) void resize_copy_kernel(const unsigned char* __restrict__ src, const int* __restrict__ windows, Geom g,
                                                         const float* __restrict__ lut, Out o) {
  __shared__ float s_lut[kLut];
  load_lut(s_lut, lut, o.f32 != nullptr);
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= g.h_win * g.w_win) return;
  const int y = i / g.w_win, x = i - y * g.w_win;
  for (int n = blockIdx.y; n < g.N; n += gridDim.y) {
    const int2 win = window_of(windows, g, n);
    const unsigned char* p = src + ((n * g.Hs + win.x + y) * g.Ws + win.y + x) * 3;
    emit(o, g, s_lut, n, y, x, p[0], p[1], p[2]);
  }
}

// out[n, y, x] = src[n, rows[top + y], cols[left + x]] * ratio.  grid = (ceil(h_win w_win / NT), min(N, 65535)).
__global__ __launch_bounds__(NT) void disp_nearest_kernel(const float* __restrict__ src, const int* __restrict__ rows,
                                                          const int* __restrict__ cols, const int* __restrict__ windows, Geom g, float ratio,
                                                          float* __restrict__ out) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= g.h_win * g.w_win) return;
  const int y = i / g.w_win, x = i - y * g.w_win;
  for (int n = blockIdx.y; n < g.N; n += gridDim.y) {
    const int2 win = window_of(windows, g, n);
    const int r = min(max(rows[win.x + y], 0), g.Hs - 1), c = min(max(cols[win.y + x], 0), g.Ws - 1);
    out[n * g.h_win * g.w_win + i] = src[(n * g.Hs + r) * g.Ws + c] * ratio;
  }
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// n * a * b * per < 2^31 without forming a product that could overflow (n >= 0, a, b, per > 0)
bool fits31(long long n, int a, int b, int per) {
  const long long lim = (1LL << 31) - 1, ab = (long long)a * b;
  return ab <= lim / per && n <= lim / per / ab;
}

// sizes a pass takes: from n to out with n <= 4 out and out <= 4 n
bool scale_ok(int n, int out) { return (long long)n <= (long long)kMaxScale * out && (long long)out <= (long long)kMaxScale * n; }

dim3 grid_of(int pixels, int N) { return dim3((unsigned)mode::cdiv(pixels, NT), (unsigned)std::min(N, 65535)); }

}  // namespace

extern "C" size_t mode_images_u8_resize_pil_workspace_bytes(int N, int Hs, int Ws, int H, int W, int h_win, int w_win) {
  if (N <= 0 || Hs <= 0 || Ws <= 0 || H <= 0 || W <= 0 || h_win <= 0 || w_win <= 0 || h_win > H || w_win > W) return 0;
  if (Hs == H || Ws == W) return 0;  // at most one pass: no intermediate image
  return (size_t)N * (size_t)Hs * (size_t)w_win * 3;
}

extern "C" int mode_images_u8_resize_pil(const uint8_t* images_u8, const int32_t* tab_w, int ksize_w, const int32_t* tab_h, int ksize_h,
                                         const float* lut, const int32_t* windows, int per_window, int split, int N, int Hs, int Ws, int H,
                                         int W, int h_win, int w_win, uint8_t* out_u8, float* out, void* workspace,
                                         size_t workspace_bytes, mode_stream_t stream) {
  const char* who = "mode_images_u8_resize_pil";
  MODE_REQUIRE(N >= 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0, MODE_ERR_BAD_ARG, "%s: bad size %d x %d x %d -> %d x %d", who, N, Hs, Ws, H, W);
  MODE_REQUIRE(h_win > 0 && w_win > 0 && h_win <= H && w_win <= W, MODE_ERR_BAD_ARG,
               "%s: a window of %d x %d does not lie inside the %d x %d image", who, h_win, w_win, H, W);
  MODE_REQUIRE(per_window >= 1 && (split == 0 || split == 1) && (!split || N % per_window == 0), MODE_ERR_BAD_ARG,
               "%s: %d images per window (split %d) for %d images", who, per_window, split, N);
  MODE_REQUIRE(scale_ok(Hs, H) && scale_ok(Ws, W), MODE_ERR_UNSUPPORTED, "%s: %d x %d -> %d x %d is beyond a factor of %d along an axis", who,
               Hs, Ws, H, W, kMaxScale);
  MODE_REQUIRE(fits31(N, Hs, Ws, 3) && fits31(N, Hs, W, 3) && fits31(N, H, W, 3), MODE_ERR_BAD_ARG,
               "%s: bad size %d x %d x %d -> %d x %d (too large: 3 N Hs max(Ws, W) or 3 N H W >= 2^31)", who, N, Hs, Ws, H, W);
  const bool pass_w = Ws != W, pass_h = Hs != H;
  MODE_REQUIRE((!pass_w || (ksize_w >= 1 && ksize_w <= kMaxTaps)) && (!pass_h || (ksize_h >= 1 && ksize_h <= kMaxTaps)), MODE_ERR_BAD_ARG,
               "%s: tables of %d and %d taps (1 .. %d)", who, ksize_w, ksize_h, kMaxTaps);
  if (N == 0) return MODE_OK;
  MODE_REQUIRE(images_u8 && (!pass_w || tab_w) && (!pass_h || tab_h), MODE_ERR_BAD_ARG, "%s: null pointer", who);
  MODE_REQUIRE(out_u8 || out, MODE_ERR_BAD_ARG, "%s: null pointer (both outputs)", who);
  MODE_REQUIRE(!out || lut, MODE_ERR_BAD_ARG, "%s: null pointer (the fp32 output needs the table)", who);
  MODE_REQUIRE(aligned(tab_w, 4) && aligned(tab_h, 4) && aligned(windows, 4) && aligned(lut, 4) && aligned(out, 4), MODE_ERR_BAD_ARG,
               "%s: tables, windows and the fp32 output must be 4-byte aligned", who);
  const size_t need = mode_images_u8_resize_pil_workspace_bytes(N, Hs, Ws, H, W, h_win, w_win);
  MODE_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), MODE_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who,
               workspace ? workspace_bytes : (size_t)0, need);
  const Geom g{N, Hs, Ws, H, W, h_win, w_win, per_window, split};
  const Tab tw{tab_w, 2 + ksize_w, Ws}, th{tab_h, 2 + ksize_h, Hs};
  const Out o{out_u8, out};
  unsigned char* mid = static_cast<unsigned char*>(workspace);
  hipStream_t st = mode::as_stream(stream);
  const dim3 final_grid = grid_of(h_win * w_win, N);
  if (pass_w && pass_h) {
    hipLaunchKernelGGL(resize_h_kernel<false>, grid_of(Hs * w_win, N), dim3(NT), 0, st, images_u8, tw, th, windows, g, lut, o, mid);
    const int rc = mode::check_launch(who);
    if (rc != MODE_OK) return rc;
    hipLaunchKernelGGL(resize_v_kernel<true>, final_grid, dim3(NT), 0, st, mid, th, windows, g, lut, o);
  } else if (pass_w) {
    hipLaunchKernelGGL(resize_h_kernel<true>, final_grid, dim3(NT), 0, st, images_u8, tw, th, windows, g, lut, o, mid);
  } else if (pass_h) {
    hipLaunchKernelGGL(resize_v_kernel<false>, final_grid, dim3(NT), 0, st, images_u8, th, windows, g, lut, o);
  } else {
    hipLaunchKernelGGL(resize_copy_kernel, final_grid, dim3(NT), 0, st, images_u8, windows, g, lut, o);
  }
  return mode::check_launch(who);
}

extern "C" int mode_disp_resize_nearest(const float* disp, const int32_t* rows, const int32_t* cols, const int32_t* windows, int N, int Hs,
                                        int Ws, int H, int W, int h_win, int w_win, float ratio, float* out, mode_stream_t stream) {
  const char* who = "mode_disp_resize_nearest";
  MODE_REQUIRE(N >= 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0, MODE_ERR_BAD_ARG, "%s: bad size %d x %d x %d -> %d x %d", who, N, Hs, Ws, H, W);
  MODE_REQUIRE(h_win > 0 && w_win > 0 && h_win <= H && w_win <= W, MODE_ERR_BAD_ARG,
               "%s: a window of %d x %d does not lie inside the %d x %d map", who, h_win, w_win, H, W);
  MODE_REQUIRE(fits31(N, Hs, Ws, 1) && fits31(N, H, W, 1), MODE_ERR_BAD_ARG,
               "%s: bad size %d x %d x %d -> %d x %d (too large: N Hs Ws or N H W >= 2^31)", who, N, Hs, Ws, H, W);
  if (N == 0) return MODE_OK;
  MODE_REQUIRE(disp && rows && cols && out, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  MODE_REQUIRE(aligned(disp, 4) && aligned(rows, 4) && aligned(cols, 4) && aligned(windows, 4) && aligned(out, 4), MODE_ERR_BAD_ARG,
               "%s: maps, tables and windows must be 4-byte aligned", who);
  const Geom g{N, Hs, Ws, H, W, h_win, w_win, 1, 0};
  hipLaunchKernelGGL(disp_nearest_kernel, grid_of(h_win * w_win, N), dim3(NT), 0, mode::as_stream(stream), disp, rows, cols, windows, g, ratio,
                     out);
  return mode::check_launch(who);
}
