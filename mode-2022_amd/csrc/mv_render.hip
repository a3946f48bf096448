// Novel-view rendering (include/mode_hip_mvrender.h): a panorama is lifted by its depth map and splatted into T target views.
// The z-buffer is DESIGN 28's -- the smallest range rho that lands on a target pixel -- and each target pixel then names the reference
// pixel it shows: the owner of its own key (DIRECT), or with fill = 1 the owner of the nearest key of its 3 x 3 neighbourhood where it
// holds nothing itself or holds a surface that a nearer one hides (FILLED).  The colour is that pixel's, copied (SPLAT), or the
// bilinear value of the image where the target pixel's own ray at that range falls back into the reference (RESAMPLE).
//
// Four launches whatever F, T and C are:
//   launch 1  the F T H W 64-bit keys and the F T H W 32-bit owners = all ones, one mode::fill_words over both (they are adjacent)
//   launch 2  splat: mv_visibility.hip's, one thread per reference pixel with the target loop inside (land() of mv_splat_internal.h),
//             atomicMin on the bit pattern of the fp64 rho; rho and the landing index of every pixel-target pair go to the workspace
//   launch 3  owners: one thread per pixel-target pair; a pair whose stored rho is its landing pixel's key puts its pixel index there
//             with atomicMin, so among equal ranges the smallest index owns the pixel
//   launch 4  resolve: one thread per target pixel and view (the views along gridDim.y, so that the pose is uniform in a workgroup and
//             is read from the kernel arguments with scalar loads): the 1 or 9 keys, the class, hit / range / index, and the C colours
// Integer minima only: the same inputs give the same bits on any stream.  The poses travel in the kernel arguments.
#include "mode_hip_mvrender.h"
#include "mv_splat_internal.h"

static_assert(MODE_MVR_HIT_DIRECT == 1 && MODE_MVR_HIT_FILLED == 2 && MODE_MVR_HIT_RESAMPLED == 4, "hit is a class plus one flag");

namespace {

constexpr int kMaxC = MODE_MVR_MAX_CHANNELS;
constexpr unsigned kNoOwner = ~0u;

// n_px = F H W reference pixels; pair (f, t, h, w) has the index (f T + t) H W + h W + w.
__global__ __launch_bounds__(NT) void mvr_splat_kernel(const float* __restrict__ depth, Poses poses, int T, int H, int W, int n_px,
                                                       unsigned long long* __restrict__ keys, double* __restrict__ rho,
                                                       int* __restrict__ at) {
  const int HW = H * W;
  for (int idx = blockIdx.x * NT + threadIdx.x; idx < n_px; idx += gridDim.x * NT) {
    const int f = idx / HW, r = idx - f * HW;
    const int h = r / W, w = r - h * W;
    const Dir n = pixel_dir(h, w, H, W);
    const float d = depth[idx];
    for (int tv = 0; tv < T; ++tv) {
      const int plane = (f * T + tv) * HW;  // < F T H W < 2^31
      const Landing l = land(d, n, poses.p[tv], H, W);
      if (l.at >= 0) atomicMin(keys + plane + l.at, (unsigned long long)__double_as_longlong(l.rho));
      rho[plane + r] = l.rho;
      at[plane + r] = l.at;
    }
  }
}

// n = F T H W pixel-target pairs.  A pair reads back the rho it stored, so the pair that set a key compares equal to it.
__global__ __launch_bounds__(NT) void mvr_owner_kernel(const unsigned long long* __restrict__ keys, const double* __restrict__ rho,
                                                       const int* __restrict__ at, int HW, int n, unsigned* __restrict__ owner) {
  for (int idx = blockIdx.x * NT + threadIdx.x; idx < n; idx += gridDim.x * NT) {
    const int a = at[idx];
    if (a < 0 || a >= HW) continue;
    const int r = idx % HW, plane = idx - r;
    if (keys[plane + a] == (unsigned long long)__double_as_longlong(rho[idx])) atomicMin(owner + plane + a, (unsigned)r);
  }
}

// planes = F T target planes along gridDim.y, H W pixels of one plane along gridDim.x.  one_tol = 1 + tol, formed in fp64 on the host.
// The second launch bound asks for 4 waves per SIMD: without it the kernel takes 129 VGPRs, one register over that occupancy.
__global__ __launch_bounds__(NT, 4) void mvr_resolve_kernel(const float* __restrict__ image, Poses poses,
                                                            const unsigned long long* __restrict__ keys, const unsigned* __restrict__ owner,
                                                            int T, int C, int H, int W, int planes, double one_tol, int fill, int mode,
                                                            float* __restrict__ out, unsigned char* __restrict__ hit,
                                                            float* __restrict__ range, int* __restrict__ index) {
  const int HW = H * W;
  for (int pl = blockIdx.y; pl < planes; pl += gridDim.y) {
    const int f = pl / T;
    const double* __restrict__ P = poses.p[pl - f * T];
    const int plane = pl * HW;  // < F T H W < 2^31
    const float* __restrict__ img = image + (size_t)f * C * HW;
    float* __restrict__ o = out + (size_t)pl * C * HW;
    for (int p = blockIdx.x * NT + threadIdx.x; p < HW; p += gridDim.x * NT) {
      const int y = p / W, x = p - y * W;
      const unsigned long long k = keys[plane + p];
      unsigned long long zc = kEmpty;
      int held = p;  // the target pixel whose key is zc
      int cls = MODE_MVR_HIT_NONE;
      if (!fill) {
        if (k != kEmpty) {
          cls = MODE_MVR_HIT_DIRECT;
          zc = k;
        }
      } else {
        unsigned long long zn = kEmpty;
        int first = p;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
          int yy = y + dy;
          yy = yy < 0 ? yy + H : (yy >= H ? yy - H : yy);
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) {
            const int xx = x + dx;
            if (xx < 0 || xx > W - 1) continue;
            const unsigned long long kk = keys[plane + yy * W + xx];
            if (kk < zn) {
              zn = kk;
              first = yy * W + xx;
            }
          }
        }
        if (k != kEmpty && __longlong_as_double((long long)k) <= one_tol * __longlong_as_double((long long)zn)) {
          cls = MODE_MVR_HIT_DIRECT;
          zc = k;
        } else if (zn != kEmpty) {
          cls = MODE_MVR_HIT_FILLED;
          zc = zn;
          held = first;
        }
      }
      int from = -1;
      if (cls != MODE_MVR_HIT_NONE) {
        const unsigned own = owner[plane + held];  // a key that is not empty has an owner: the pair that set it
        if (own < (unsigned)HW) from = (int)own;
        else cls = MODE_MVR_HIT_NONE;
      }
      bool resampled = false;
      Geo g;
      if (mode == MODE_MVR_RESAMPLE && cls != MODE_MVR_HIT_NONE) {
        // the target pixel's own ray at range zc, back in the reference's frame: X = A^T (zc n - o)
        const Dir n = pixel_dir(y, x, H, W);
        const double z = __longlong_as_double((long long)zc);
        const double dx = z * n.x - P[3], dy = z * n.y - P[7], dz = z * n.z - P[11];
        const double Xx = P[0] * dx + P[4] * dy + P[8] * dz;
        const double Xy = P[1] * dx + P[5] * dy + P[9] * dz;
        const double Xz = P[2] * dx + P[6] * dy + P[10] * dz;
        const double s2 = Xy * Xy + Xz * Xz;
        const double r = sqrt(Xx * Xx + s2);
        if (r > 0.0) {
          const double phi = asin(Xx / r);
          const double theta = atan2(Xy, Xz);
          const double u = (kPi / 2 - phi) * (double)W / kPi - 0.5;
          const double v = (kPi - theta) * (double)H / (2.0 * kPi) - 0.5;
          if (u >= 0.0 && u <= (double)(W - 1) && v == v) {
            const double fv = floor(v);
            int x0 = (int)floor(u);
            x0 = x0 < W - 2 ? x0 : W - 2;
            const int y0 = (int)fv;  // -1 .. H - 1
            g.x0 = x0;
            g.ya = ((y0 % H) + H) % H;
            g.yb = g.ya + 1 == H ? 0 : g.ya + 1;
            g.t = (float)(u - (double)x0);
            g.q = (float)(v - fv);
            resampled = true;
          }
        }
      }
      hit[plane + p] = (unsigned char)(cls | (resampled ? MODE_MVR_HIT_RESAMPLED : 0));
      if (range) range[plane + p] = cls != MODE_MVR_HIT_NONE ? (float)__longlong_as_double((long long)zc) : __builtin_inff();
      if (index) index[plane + p] = from;
      if (resampled) {
        const int a = g.ya * W + g.x0, b = g.yb * W + g.x0;
        for (int c = 0; c < C; ++c) {
          const float* __restrict__ pc = img + c * HW;
          const float r00 = pc[a], r01 = pc[a + 1], r10 = pc[b], r11 = pc[b + 1];
          const float top = (1.f - g.t) * r00 + g.t * r01, bot = (1.f - g.t) * r10 + g.t * r11;
          o[c * HW + p] = (1.f - g.q) * top + g.q * bot;
        }
      } else {
        for (int c = 0; c < C; ++c) o[c * HW + p] = from >= 0 ? img[c * HW + from] : 0.f;
      }
    }
  }
}

}  // namespace

extern "C" int mode_mvrender_version(void) { return MODE_MVRENDER_VERSION; }

// The four parts of the workspace, each 16-byte aligned: keys (8 n), owners (4 n) -- adjacent, one fill --, rho (8 n), landing indices (4 n).
extern "C" size_t mode_mvrender_workspace_bytes(int T, int F, int H, int W) {
  if (T < 1 || T > kMaxS || F < 1 || H < 3 || W < 3 || 3ll * F * T * H * W >= (1ll << 31)) return 0;
  const size_t n = (size_t)F * T * H * W;
  return 2 * part(8 * n) + 2 * part(4 * n);
}

extern "C" int mode_mv_render(const float* image, const float* depth, const double* poses, int T, int F, int C, int H, int W, double tol,
                              int fill, int mode, void* workspace, size_t workspace_bytes, float* out, unsigned char* hit, float* range,
                              int* index, mode_stream_t stream) {
  const char* who = "mode_mv_render";
  MODE_REQUIRE(image && out && hit, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  MODE_REQUIRE(C >= 1 && C <= kMaxC, MODE_ERR_BAD_ARG, "%s: C = %d channels (1 .. %d)", who, C, kMaxC);
  // The family's own checks of the sizes and the poses, in the family's words; as in mode_mv_visibility the depth stands in for the
  // images of the loss, and the loss's bound 3 F T H W < 2^31 covers the 32-bit indices of the planes here.
  Prm p;
  Poses ps;
  int tiles_w, tiles;
  const mode_photometric_params no_colour = {};
  int rc = check_common(who, depth, depth, depth, poses, T, F, H, W, &no_colour, p, ps, tiles_w, tiles);
  if (rc != MODE_OK) return rc;
  MODE_REQUIRE(std::isfinite(tol) && tol >= 0.0, MODE_ERR_BAD_ARG, "%s: tol = %g must be finite and >= 0", who, tol);
  MODE_REQUIRE(fill == 0 || fill == 1, MODE_ERR_BAD_ARG, "%s: fill = %d (0 or 1)", who, fill);
  MODE_REQUIRE(mode == MODE_MVR_SPLAT || mode == MODE_MVR_RESAMPLE, MODE_ERR_BAD_ARG, "%s: mode = %d (%d: splat, %d: resample)", who, mode,
               MODE_MVR_SPLAT, MODE_MVR_RESAMPLE);
  MODE_REQUIRE((long long)C * F * T * H * W < (1ll << 31), MODE_ERR_UNSUPPORTED,
               "%s: an output of %d x %d x %d x %d x %d elements: 32-bit indices need C F T H W < 2^31", who, F, T, C, H, W);
  rc = check_workspace(who, workspace, workspace_bytes, mode_mvrender_workspace_bytes(T, F, H, W));
  if (rc != MODE_OK) return rc;
  const size_t n = (size_t)F * T * H * W;
  char* base = static_cast<char*>(workspace);
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(base);
  unsigned* owner = reinterpret_cast<unsigned*>(base + part(8 * n));
  double* rho = reinterpret_cast<double*>(base + part(8 * n) + part(4 * n));
  int* at = reinterpret_cast<int*>(base + 2 * part(8 * n) + part(4 * n));
  static_assert(kEmpty == ~0ull && kNoOwner == ~0u, "one fill pattern for the keys and the owners");
  hipStream_t st = mode::as_stream(stream);
  rc = mode::fill_words(keys, 0xffffffffu, part(8 * n) / 4 + n, st, who);  // (a kernel, not a runtime fill: common.h)
  if (rc != MODE_OK) return rc;
  const int n_px = F * H * W, HW = H * W, planes = F * T;
  hipLaunchKernelGGL(mvr_splat_kernel, dim3(grid_for(n_px)), dim3(NT), 0, st, depth, ps, T, H, W, n_px, keys, rho, at);
  hipLaunchKernelGGL(mvr_owner_kernel, dim3(grid_for((long long)n)), dim3(NT), 0, st, keys, rho, at, HW, (int)n, owner);
  hipLaunchKernelGGL(mvr_resolve_kernel, dim3(grid_for(HW), std::min(planes, 1024)), dim3(NT), 0, st, image, ps, keys, owner, T, C, H, W,
                     planes, 1.0 + tol, fill, mode, out, hit, range, index);
  return mode::check_launch(who);
}
