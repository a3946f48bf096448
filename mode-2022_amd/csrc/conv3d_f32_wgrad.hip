// Weight gradient of the 3x3x3 convolution (pad 1, stride 1 | 2) on the fp32 MFMA, gfx950; the forward kernels are in
// conv3d_f32_fwd.hip, the C entries in conv3d.hip.  Also the reduction of the split-K partials, which the split-bf16 weight
// gradients (conv3d_split_wgrad.hip, conv3d_split_wgrad_s2.hip) share: they write their partials in the same layout.
//
// Backward w.r.t. the weight:  gW[o][c][tap] = sum_{b,q} gy[b,o,q] * x[b,c, S*q + k - 1]   (q = output voxel, S = stride).
//   D[i = o][j = c] per tap;  A[i = o][k = voxel] = gy tile (LDS),  B[k = voxel][j = c] = x tile shifted by the tap (LDS).
// A workgroup owns a 32x32 (o,c) block and a slice of the spatial tiles (WTH rows x 32 output voxels); its 4 waves share
// the A fragment and split the 27 taps (7,7,7,6 accumulators).  Split-K partials are reduced in a fixed order.
// The same kernel serves ConvTranspose3d (k3 s2 p1 op1): gWt[ci][co][k] = sum_q x_in[ci,q] * gy_out[co, 2q + k - 1], i.e.
// call it with (gy := transposed-conv input, x := transposed-conv output gradient, S = 2).
#include "common.h"
#include <cstdlib>
#include <string>

#include "conv3d_internal.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int NT = 256;

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

struct WDims {
  int B, Ci, Co, D, H, W;  // x volume (high resolution)
  int Do, Ho, Wo;          // gy volume
  int nWt, nHt;
  int T;  // spatial tiles in total
  int S;  // split-K slices
  int MTo, MTc;
};

template <int S, int WTH>
struct WGeom {
  static constexpr int XR = (WTH - 1) * S + 3;          // x rows per tile
  static constexpr int XW = (S == 1) ? 34 : 65;         // x columns per tile
  static constexpr int XP0 = 3 * XR * XW;
  static constexpr int XPLANE = XP0 | 1;                // odd -> lanes (= channels) hit distinct banks
  static constexpr int GPLANE = WTH * 32 + 1;
  static constexpr size_t LDS = (size_t)(32 * XPLANE + 32 * GPLANE) * sizeof(float);
};

template <int S, int WTH>
__global__ __launch_bounds__(NT) void conv3d_bwd_weight_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                               float* __restrict__ part, WDims d) {
  using G = WGeom<S, WTH>;
  constexpr int XR = G::XR, XW = G::XW, XPLANE = G::XPLANE, GPLANE = G::GPLANE;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xl = lds;                 // [32][XPLANE]
  float* gl = lds + 32 * XPLANE;   // [32][GPLANE]
  const int s = blockIdx.x, ob = blockIdx.y, cb = blockIdx.z;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long long HW = (long long)d.H * d.W;
  const long long DHW = (long long)d.D * HW;
  const long long oHW = (long long)d.Ho * d.Wo;
  const long long oDHW = (long long)d.Do * oHW;

  f32x16 acc[7];
  int toff[7];
#pragma unroll
  for (int t = 0; t < 7; ++t) {
    acc[t] = (f32x16){0};
    const int tap = wave + 4 * t;  // < 27 except wave 3, t = 6
    toff[t] = (tap / 9) * (XR * XW) + ((tap / 3) % 3) * XW + (tap % 3);
  }
  const bool last_valid = (wave + 24) < 27;

  for (int tt = s; tt < d.T; tt += d.S) {
    int t = tt;
    const int wt = t % d.nWt;
    t /= d.nWt;
    const int ht = t % d.nHt;
    t /= d.nHt;
    const int qd = t % d.Do;
    const int b = t / d.Do;
    const int w0 = wt * 32, h0 = ht * WTH;  // output (gy) coordinates
    const float* xb = x + ((long long)b * d.Ci + cb * 32) * DHW;
    const float* gb = gy + ((long long)b * d.Co + ob * 32) * oDHW;
    {
      // Branch-free row staging (see conv3d_kernel): the x tile is 32*3*XR rows of XW floats; a half-wave loads 32
      // consecutive columns of a row per instruction, 8 loads per thread in flight; leftover columns one per thread.
      constexpr int NROWS = 32 * 3 * XR;
      constexpr int NG = (XW - 1) / 32;          // full 32-column groups per row: 1 (34 cols) or 2 (65 cols)
      constexpr int NLEFT = XW - 32 * NG;        // 2 or 1 leftover columns
      constexpr int WNF = 8;                     // loads in flight per thread and batch (24 drops the kernel to one wave per SIMD: 1.9 vs 1.2 ms)
      const int hwv = tid >> 5, l32 = tid & 31;
#pragma unroll 1
      for (int kb = 0; kb < NROWS * NG; kb += 8 * WNF) {
        float t8[WNF];
#pragma unroll
        for (int j = 0; j < WNF; ++j) {
          const int item = kb + j * 8 + hwv;
          const int r = item / NG, g = item - r * NG;
          const int c = r / (3 * XR), rem = r - c * (3 * XR);
          const int gd = qd * S + rem / XR - 1, gh = h0 * S + rem % XR - 1;
          const int wx = (NLEFT == 2 ? 1 : 0) + 32 * g + l32;
          const int gw = w0 * S + wx - 1;
          const bool ok = item < NROWS * NG && cb * 32 + c < d.Ci && gd >= 0 && gd < d.D && gh >= 0 && gh < d.H && gw >= 0 && gw < d.W;
          const float v = xb[ok ? c * DHW + gd * HW + gh * d.W + gw : 0];
          t8[j] = ok ? v : 0.f;
        }
#pragma unroll
        for (int j = 0; j < WNF; ++j) {
          const int item = kb + j * 8 + hwv;
          const int r = item / NG, g = item - r * NG;
          const int c = r / (3 * XR), rem = r - c * (3 * XR);
          const int wx = (NLEFT == 2 ? 1 : 0) + 32 * g + l32;
          if (item < NROWS * NG) xl[c * XPLANE + rem * XW + wx] = t8[j];
        }
      }
#pragma unroll 1
      for (int item = tid; item < NROWS * NLEFT; item += NT) {
        const int r = item / NLEFT, side = item - r * NLEFT;
        const int c = r / (3 * XR), rem = r - c * (3 * XR);
        const int gd = qd * S + rem / XR - 1, gh = h0 * S + rem % XR - 1;
        const int wx = (NLEFT == 2) ? (side ? XW - 1 : 0) : XW - 1;
        const int gw = w0 * S + wx - 1;
        const bool ok = cb * 32 + c < d.Ci && gd >= 0 && gd < d.D && gh >= 0 && gh < d.H && gw >= 0 && gw < d.W;
        const float v = xb[ok ? c * DHW + gd * HW + gh * d.W + gw : 0];
        xl[c * XPLANE + rem * XW + wx] = ok ? v : 0.f;
      }
      constexpr int GROWS = 32 * WTH;  // (output channel, row) pairs of the gy tile
#pragma unroll 1
      for (int kb = 0; kb < GROWS; kb += 64) {
        float t8[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int r = kb + j * 8 + hwv;
          const int o = r / WTH, gh = h0 + r % WTH, gw = w0 + l32;
          const bool ok = r < GROWS && ob * 32 + o < d.Co && gh < d.Ho && gw < d.Wo;
          const float v = gb[ok ? o * oDHW + qd * oHW + gh * d.Wo + gw : 0];
          t8[j] = ok ? v : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int r = kb + j * 8 + hwv;
          if (r < GROWS) gl[(r / WTH) * GPLANE + (r % WTH) * 32 + l32] = t8[j];
        }
      }
    }
    __syncthreads();
    const float* ap = gl + (lane & 31) * GPLANE + (lane >> 5);
    const float* bp = xl + (lane & 31) * XPLANE + (lane >> 5) * S;
#pragma unroll
    for (int row = 0; row < WTH; ++row) {
#pragma unroll 4
      for (int ks = 0; ks < 16; ++ks) {
        const float a = ap[row * 32 + 2 * ks];
        const float* bq = bp + row * S * XW + 2 * ks * S;
#pragma unroll
        for (int t6 = 0; t6 < 6; ++t6) acc[t6] = mfma32(a, bq[toff[t6]], acc[t6]);
        if (last_valid) acc[6] = mfma32(a, bq[toff[6]], acc[6]);
      }
    }
    __syncthreads();
  }

  float* pb = part + (((long long)s * d.MTo + ob) * d.MTc + cb) * (27 * 1024);
#pragma unroll
  for (int t = 0; t < 7; ++t) {
    const int tap = wave + 4 * t;
    if (tap < 27) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int i = (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
        pb[tap * 1024 + i * 32 + (lane & 31)] = acc[t][q];
      }
    }
  }
}

// Stride-2 variant, software pipelined.  The generic kernel above alternates "stage a tile" and "27 x 16 MFMAs on it" with a
// barrier in between, and at two workgroups per CU (75 KB of LDS each) there is nothing else to hide the staging behind:
// 37 TFLOP/s.  Here the NEXT tile travels global -> registers while the MFMAs of the current one run (78 loads per thread in
// flight, issued before the k-loop, consumed after it), so a step costs max(load, MFMA) + the LDS stores.  The item -> (channel,
// row, column group) map is chosen so that everything but the half-wave's channel is a compile-time constant: a tile needs 9
// row offsets, 2 column offsets and an 11-bit validity mask, the 72 addresses are sums of those.
// OB = output-channel blocks per workgroup (256 threads each): with OB = 2 the two blocks of a 64-channel gy share one staged x
// tile -- half the loads, LDS stores and prefetch registers per thread for the same MFMAs.
template <int OB>
__global__ __launch_bounds__(NT * OB, 2) void conv3d_bwd_weight_s2_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                                     float* __restrict__ part, WDims d) {
  using G = WGeom<2, 1>;
  constexpr int XR = G::XR, XW = G::XW, XPLANE = G::XPLANE, GPLANE = G::GPLANE;
  static_assert(XR == 3 && XW == 65, "item map below assumes the 3 x 3 x 65 tile");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xl = lds;                 // [32][XPLANE]
  float* gl = lds + 32 * XPLANE;   // [32 * OB][GPLANE]
  constexpr int NTH = NT * OB, HWV = 8 * OB;                 // threads, half-waves
  constexpr int NQ = 4 / OB, NX = 18 * NQ;                   // channels per half-wave, x items per thread
  constexpr int NE = (288 + NTH - 1) / NTH;                  // column-64 items per thread
  const int s = blockIdx.x, cb = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = (tid >> 6) & 3, oh = tid >> 8;            // tap group, output-channel block of this wave
  const int ob0 = blockIdx.y * OB, ob = ob0 + oh;
  const int hwv = tid >> 5, l32 = tid & 31;
  const int HW = d.H * d.W, DHW = d.D * HW;          // (host guarantees Ci * DHW < 2^29)
  const int oHW = d.Ho * d.Wo, oDHW = d.Do * oHW;

  f32x16 acc[7];
  int toff[7];
#pragma unroll
  for (int t = 0; t < 7; ++t) {
    acc[t] = (f32x16){0};
    const int tap = min(wave + 4 * t, 26);  // wave 3, t = 6 would be tap 27: it repeats tap 26 and drops the result
    toff[t] = (tap / 9) * (XR * XW) + ((tap / 3) % 3) * XW + (tap % 3);
  }

  // x tile = 288 (channel, depth, row) rows of 65 columns.  Columns 0..63: item jj of half-wave hwv is channel hwv + 8 * (jj / 18),
  // row (jj % 18) / 2, column group jj & 1.  Column 64: one item per thread (+ 32 threads a second one).  gy tile: 32 x 32.
  float px[NX], pe[NE], pg[4];
  unsigned chan_ok = 0;
#pragma unroll
  for (int q = 0; q < NQ; ++q) chan_ok |= (cb * 32 + hwv + HWV * q < d.Ci ? 1u : 0u) << q;
  const bool all_chan = cb * 32 + 32 <= d.Ci;  // (block-uniform)
  const int e_r0 = tid, e_r1 = tid + NTH;  // rows of the column-64 items (the second one only with OB = 1)
  const int e_c0 = min(e_r0, 287) / 9, e_m0 = min(e_r0, 287) - 9 * e_c0, e_c1 = min(e_r1, 287) / 9, e_m1 = min(e_r1, 287) - 9 * e_c1;

  // issues the loads of tile tt, returns its validity mask (bits 0..8 rows, 9..10 column groups, 11 column 64, 12 gy column)
  auto prefetch = [&](int tt) -> unsigned {
    int t = tt;
    const int wt = t % d.nWt;
    t /= d.nWt;
    const int ht = t % d.nHt;
    t /= d.nHt;
    const int qd = t % d.Do;
    const int b = t / d.Do;
    const int w0 = wt * 32, h0 = ht;
    const float* xb = x + ((long long)b * d.Ci + cb * 32) * (long long)DHW;
    const float* gb = gy + ((long long)b * d.Co + ob0 * 32) * (long long)oDHW;
    unsigned m = 0;
    int rowoff[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) {
      const int gd = 2 * qd + r / 3 - 1, gh = 2 * h0 + r % 3 - 1;
      const bool ok = gd >= 0 && gd < d.D && gh >= 0 && gh < d.H;
      rowoff[r] = ok ? gd * HW + gh * d.W : 0;
      m |= (ok ? 1u : 0u) << r;
    }
    const int gw0 = 2 * w0 + l32 - 1, gw1 = gw0 + 32, gw2 = 2 * w0 + 63;
    m |= (gw0 >= 0 && gw0 < d.W ? 1u : 0u) << 9;
    m |= (gw1 < d.W ? 1u : 0u) << 10;
    m |= (gw2 < d.W ? 1u : 0u) << 11;
    m |= (w0 + l32 < d.Wo ? 1u : 0u) << 12;
    const int cbase = hwv * DHW;
    if (all_chan && (m & 0x1ffu) == 0x1ffu) {
      // interior tile (every row and channel exists -- all but the first depth / row of a sample): no per-item masks, the two
      // column groups read a clamped column and are masked by one select each at the LDS store (PMC: the general form below
      // costs 4.9 VALU + 3.4 SALU instructions per MFMA)
      m |= 1u << 13;
      const int c0 = cbase + ((m >> 9) & 1 ? gw0 : 0), c1 = cbase + ((m >> 10) & 1 ? gw1 : 0);
#pragma unroll
      for (int jj = 0; jj < NX; ++jj) {
        const int q = jj / 18, r = (jj % 18) / 2, g = jj & 1;
        px[jj] = xb[(g ? c1 : c0) + q * HWV * DHW + rowoff[r]];
      }
    } else {
#pragma unroll
      for (int jj = 0; jj < NX; ++jj) {
        const int q = jj / 18, r = (jj % 18) / 2, g = jj & 1;
        const bool ok = ((chan_ok >> q) & 1) && ((m >> r) & 1) && ((m >> (9 + g)) & 1);
        const int off = cbase + q * HWV * DHW + rowoff[r] + (g ? gw1 : gw0);
        px[jj] = xb[ok ? off : 0];
      }
    }
    {
      const int gd0 = 2 * qd + e_m0 / 3 - 1, gh0 = 2 * h0 + e_m0 % 3 - 1;
      const bool ok0 = e_r0 < 288 && ((m >> e_m0) & 1) && ((m >> 11) & 1) && cb * 32 + e_c0 < d.Ci;
      pe[0] = xb[ok0 ? e_c0 * DHW + gd0 * HW + gh0 * d.W + gw2 : 0];
      if (NE > 1) {
        const int gd1 = 2 * qd + e_m1 / 3 - 1, gh1 = 2 * h0 + e_m1 % 3 - 1;
        const bool ok1 = e_r1 < 288 && ((m >> e_m1) & 1) && ((m >> 11) & 1) && cb * 32 + e_c1 < d.Ci;
        pe[NE - 1] = xb[ok1 ? e_c1 * DHW + gd1 * HW + gh1 * d.W + gw2 : 0];
      }
    }
    const int gbase = qd * oHW + h0 * d.Wo + w0 + l32;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int o = HWV * j + hwv;  // row of the 32 * OB gy tile
      const bool ok = ((m >> 12) & 1) && ob0 * 32 + o < d.Co;
      pg[j] = gb[ok ? o * oDHW + gbase : 0];
    }
    return m;
  };
  // registers -> LDS for the tile whose mask is m (masked elements become zeros)
  auto store = [&](unsigned m) {
    float* xrow = xl + hwv * XPLANE + l32;
    if ((m >> 13) & 1) {  // interior tile: only the column masks
      const bool ok0 = (m >> 9) & 1, ok1 = (m >> 10) & 1;
#pragma unroll
      for (int jj = 0; jj < NX; ++jj) {
        const int q = jj / 18, r = (jj % 18) / 2, g = jj & 1;
        xrow[q * HWV * XPLANE + r * XW + 32 * g] = (g ? ok1 : ok0) ? px[jj] : 0.f;
      }
    } else {
#pragma unroll
      for (int jj = 0; jj < NX; ++jj) {
        const int q = jj / 18, r = (jj % 18) / 2, g = jj & 1;
        const bool ok = ((chan_ok >> q) & 1) && ((m >> r) & 1) && ((m >> (9 + g)) & 1);
        xrow[q * HWV * XPLANE + r * XW + 32 * g] = ok ? px[jj] : 0.f;
      }
    }
    if (e_r0 < 288) {
      const bool ok0 = ((m >> e_m0) & 1) && ((m >> 11) & 1) && cb * 32 + e_c0 < d.Ci;
      xl[e_c0 * XPLANE + e_m0 * XW + 64] = ok0 ? pe[0] : 0.f;
    }
    if (NE > 1 && e_r1 < 288) {
      const bool ok1 = ((m >> e_m1) & 1) && ((m >> 11) & 1) && cb * 32 + e_c1 < d.Ci;
      xl[e_c1 * XPLANE + e_m1 * XW + 64] = ok1 ? pe[NE - 1] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int o = HWV * j + hwv;
      const bool ok = ((m >> 12) & 1) && ob0 * 32 + o < d.Co;
      gl[o * GPLANE + l32] = ok ? pg[j] : 0.f;
    }
  };

  const int s_x = xcd_remap(s, d.S);  // XCD-aware tile order (neighbouring tiles share halos in one L2), see the ring kernel
  unsigned mask = 0;
  if (s_x < d.T) mask = prefetch(s_x);
  const float* ap = gl + (oh * 32 + (lane & 31)) * GPLANE + (lane >> 5);
  const float* bp = xl + (lane & 31) * XPLANE + (lane >> 5) * 2;
  for (int tt = s_x; tt < d.T; tt += d.S) {
    store(mask);
    __syncthreads();
    if (tt + d.S < d.T) mask = prefetch(tt + d.S);
    __builtin_amdgcn_sched_barrier(0);
    // operands of k-step ks+1 are read from LDS before the 7 MFMAs of k-step ks are issued (the straightforward loop waited
    // for an LDS round trip at the head of every k-step, and once more inside the branch around the 7th tap: all four waves
    // now run 7 taps -- wave 3's last one is a duplicate whose result is dropped -- and there is no branch)
    float a_n = ap[0], b_n[7];
#pragma unroll
    for (int t7 = 0; t7 < 7; ++t7) b_n[t7] = bp[toff[t7]];
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
      const float a = a_n;
      float bb[7];
#pragma unroll
      for (int t7 = 0; t7 < 7; ++t7) bb[t7] = b_n[t7];
      if (ks + 1 < 16) {
        a_n = ap[2 * (ks + 1)];
#pragma unroll
        for (int t7 = 0; t7 < 7; ++t7) b_n[t7] = bp[4 * (ks + 1) + toff[t7]];
      }
      __builtin_amdgcn_sched_barrier(0);  // (the compiler would sink these reads to their first use)
#pragma unroll
      for (int t7 = 0; t7 < 7; ++t7) acc[t7] = mfma32(a, bb[t7], acc[t7]);
    }
    __syncthreads();
  }

  float* pb = part + (((long long)s * d.MTo + (ob < d.MTo ? ob : 0)) * d.MTc + cb) * (27 * 1024);
#pragma unroll
  for (int t = 0; t < 7; ++t) {
    const int tap = wave + 4 * t;
    if (tap < 27 && ob < d.MTo) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int i = (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
        pb[tap * 1024 + i * 32 + (lane & 31)] = acc[t][q];
      }
    }
  }
}

// Stride-1 variant with a rolling depth window: a work unit is a (b, h-tile, w-tile) column times a run of DC consecutive
// depths; the three x planes d-1, d, d+1 live in an LDS ring and only plane d+1 is staged per step (the halo re-read per
// 64 output voxels drops from 408 to 136 floats per channel).  Same fragment maps and partial layout as the kernel above.
__global__ __launch_bounds__(NT) void conv3d_bwd_weight_ring_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                                    float* __restrict__ part, WDims d, int nDc, int units, int ring_dc) {
  constexpr int WTH = 2, XR = WTH + 2, XW = 34, PS = XR * XW;  // plane = 136 floats
    constexpr int XPLANE = 3 * PS + 1;                           // 409 (odd)
  constexpr int GPLANE = WTH * 32 + 1;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xl = lds;                 // [32][3 ring slots][XR][XW]
  float* gl = lds + 32 * XPLANE;   // [32][GPLANE]
  const int s = blockIdx.x, ob = blockIdx.y, cb = blockIdx.z;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long long HW = (long long)d.H * d.W;
  const long long DHW = (long long)d.D * HW;

  f32x16 acc[7];
  int kd[7], khw[7];
#pragma unroll
  for (int t = 0; t < 7; ++t) {
    acc[t] = (f32x16){0};
    const int tap = min(wave + 4 * t, 26);  // wave 3, t = 6 would be tap 27: it repeats tap 26 and drops the result (no branch)
    kd[t] = tap / 9;
    khw[t] = ((tap / 3) % 3) * XW + (tap % 3);
  }
  const int hwv = tid >> 5, l32 = tid & 31;
  const int HWi = d.H * d.W, DHWi = d.D * HWi;  // (host guarantees 32-bit element offsets within a sample)
  unsigned chan_ok = 0, gchan_ok = 0;           // x item j is channel 2 * j + (hwv >> 2), gy item j is channel 4 * j + (hwv >> 1)
#pragma unroll
  for (int j = 0; j < 16; ++j) chan_ok |= (cb * 32 + 2 * j + (hwv >> 2) < d.Ci ? 1u : 0u) << j;
#pragma unroll
  for (int j = 0; j < 8; ++j) gchan_ok |= (ob * 32 + 4 * j + (hwv >> 1) < d.Co ? 1u : 0u) << j;

  // XCD-aware: consecutive workgroup ids go round-robin over the 8 XCDs, so give every XCD a contiguous range of units --
  // neighbouring tiles share halo rows, and they only meet in an L2 if they run on the same XCD (PMC: 1.20 GB fetched per launch
  // with the plain mapping, for 0.81 GB of operands)
  for (int u = xcd_remap(s, d.S); u < units; u += d.S) {
    int t = u;
    const int dc = t % nDc;
    t /= nDc;
    const int wt = t % d.nWt;
    t /= d.nWt;
    const int ht = t % d.nHt;
    const int b = t / d.nHt;
    const int w0 = wt * 32, h0 = ht * WTH;
    const int dlo = dc * ring_dc, dhi = min(d.D, dlo + ring_dc);
    const float* xb = x + ((long long)b * d.Ci + cb * 32) * DHW;
    const float* gb = gy + ((long long)b * d.Co + ob * 32) * DHW;

    // Software pipeline over the depths of the unit: while the MFMAs of depth dd run, plane dd+2 and the gy rows of depth
    // dd+1 travel global -> registers (25 loads per thread); they are written to LDS (ring slot of plane dd-1, which is dead
    // by then) after the k-loop.  Loads are unconditional from clamped addresses, the masks are applied at the LDS store.
    const int gh_x = h0 + (hwv & 3) - 1;      // every item of a thread is the same tile row ...
    const int gw_x = w0 + l32;                // ... and column
    const bool rc_ok = gh_x >= 0 && gh_x < d.H && gw_x < d.W;
    const int xoff = (hwv >> 2) * DHWi + (rc_ok ? gh_x * d.W + gw_x : 0);  // + 2 * item * DHW + z * HW
    const int hr = tid >> 1, hside = tid & 1;  // halo item: (channel, row) = (hr >> 2, hr & 3), left / right column
    const int gh_h = h0 + (hr & 3) - 1, gw_h = hside ? w0 + 32 : w0 - 1;
    const bool h_ok = cb * 32 + (hr >> 2) < d.Ci && gh_h >= 0 && gh_h < d.H && gw_h >= 0 && gw_h < d.W;
    const int hoff = h_ok ? (hr >> 2) * DHWi + gh_h * d.W + gw_h : 0;
    const int gh_g = h0 + (hwv & 1);           // gy item j: output channel 4 * j + (hwv >> 1), row hwv & 1
    const bool g_ok = gh_g < d.H && gw_x < d.W;
    const int goff = (hwv >> 1) * DHWi + (g_ok ? gh_g * d.W + gw_x : 0);
    float px[16], ph, pg[8];
    auto load_plane = [&](int z) {
      const int zo = (z >= 0 && z < d.D ? z : 0) * HWi;
#pragma unroll
      for (int j = 0; j < 16; ++j) px[j] = xb[((chan_ok >> j) & 1) && rc_ok ? xoff + 2 * j * DHWi + zo : 0];
      ph = xb[hoff + (h_ok ? zo : 0)];
    };
    auto store_plane = [&](int z) {
      const bool zok = z >= 0 && z < d.D;
      float* dst = xl + (hwv >> 2) * XPLANE + ((z + 3) % 3) * PS + (hwv & 3) * XW + 1 + l32;
#pragma unroll
      for (int j = 0; j < 16; ++j) dst[2 * j * XPLANE] = (zok && rc_ok && ((chan_ok >> j) & 1)) ? px[j] : 0.f;
      xl[(hr >> 2) * XPLANE + ((z + 3) % 3) * PS + (hr & 3) * XW + (hside ? 33 : 0)] = (zok && h_ok) ? ph : 0.f;
    };
    auto load_gy = [&](int z) {
#pragma unroll
      for (int j = 0; j < 8; ++j) pg[j] = gb[((gchan_ok >> j) & 1) && g_ok ? goff + 4 * j * DHWi + z * HWi : 0];
    };
    auto store_gy = [&]() {
      float* dst = gl + (hwv >> 1) * GPLANE + (hwv & 1) * 32 + l32;
#pragma unroll
      for (int j = 0; j < 8; ++j) dst[4 * j * GPLANE] = (g_ok && ((gchan_ok >> j) & 1)) ? pg[j] : 0.f;
    };
    // prologue: planes dlo-1, dlo, dlo+1 and the gy rows of depth dlo
    load_plane(dlo - 1);
    load_gy(dlo);
    store_plane(dlo - 1);
    store_gy();
    load_plane(dlo);
    store_plane(dlo);
    load_plane(dlo + 1);
    store_plane(dlo + 1);
    __syncthreads();

    for (int dd = dlo; dd < dhi; ++dd) {
      const bool more = dd + 1 < dhi;
      if (more) {
        load_plane(dd + 2);
        load_gy(dd + 1);
      }
      __builtin_amdgcn_sched_barrier(0);
      int toff[7];
#pragma unroll
      for (int t7 = 0; t7 < 7; ++t7) toff[t7] = ((dd + kd[t7] + 2) % 3) * PS + khw[t7];  // depth dd + kd - 1
      const float* ap = gl + (lane & 31) * GPLANE + (lane >> 5);
      const float* bp = xl + (lane & 31) * XPLANE + (lane >> 5);
      // 32 k-steps (2 rows x 16 voxel pairs); the operands of step i+1 are read from LDS before the 7 MFMAs of step i are issued
      float a_n = ap[0], b_n[7];
#pragma unroll
      for (int t7 = 0; t7 < 7; ++t7) b_n[t7] = bp[toff[t7]];
#pragma unroll
      for (int i = 0; i < WTH * 16; ++i) {
        const float a = a_n;
        float bb[7];
#pragma unroll
        for (int t7 = 0; t7 < 7; ++t7) bb[t7] = b_n[t7];
        if (i + 1 < WTH * 16) {
          const int row = (i + 1) / 16, ks = (i + 1) % 16;
          a_n = ap[row * 32 + 2 * ks];
#pragma unroll
          for (int t7 = 0; t7 < 7; ++t7) b_n[t7] = bp[row * XW + 2 * ks + toff[t7]];
        }
        __builtin_amdgcn_sched_barrier(0);  // (the compiler would sink these reads to their first use)
#pragma unroll
        for (int t7 = 0; t7 < 7; ++t7) acc[t7] = mfma32(a, bb[t7], acc[t7]);
      }
      __syncthreads();
      if (more) {
        store_plane(dd + 2);
        store_gy();
      }
      __syncthreads();
    }
  }

  float* pb = part + (((long long)s * d.MTo + ob) * d.MTc + cb) * (27 * 1024);
#pragma unroll
  for (int t = 0; t < 7; ++t) {
    const int tap = wave + 4 * t;
    if (tap < 27) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int i = (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
        pb[tap * 1024 + i * 32 + (lane & 31)] = acc[t][q];
      }
    }
  }
}

// gw[o][c][tap] (+)= sum_s part[s][o/32][c/32][tap][o%32][c%32].  A block of 256 threads handles 32 consecutive elements of the
// partial layout: thread (e, g) sums the slices s = g, g+8, ... in order (coalesced 128-byte reads per slice), the 8 group sums
// are combined through LDS in a fixed association -- deterministic, and 8x the parallelism of one thread per element.
__global__ __launch_bounds__(256) void reduce_gw3d(const float* __restrict__ part, float* __restrict__ gw, WDims d, int accumulate) {
  __shared__ float sh[8][33];
  const long long stride = (long long)d.MTo * d.MTc * 27 * 1024;
  const int el = threadIdx.x & 31, g = threadIdx.x >> 5;
  const long long e = (long long)blockIdx.x * 32 + el;
  float a0 = 0.f, a1 = 0.f;
  if (e < stride) {
    const float* p = part + e;
    int s = g;
    for (; s + 8 < d.S; s += 16) {
      a0 += p[(long long)s * stride];
      a1 += p[(long long)(s + 8) * stride];
    }
    if (s < d.S) a0 += p[(long long)s * stride];
  }
  sh[g][el] = a0 + a1;
  __syncthreads();
  if (g == 0 && e < stride) {
    const float sum = ((sh[0][el] + sh[1][el]) + (sh[2][el] + sh[3][el])) + ((sh[4][el] + sh[5][el]) + (sh[6][el] + sh[7][el]));
    const int j = (int)(e & 31), i = (int)((e >> 5) & 31);
    long long r = e >> 10;
    const int tap = (int)(r % 27);
    r /= 27;
    const int cb = (int)(r % d.MTc), ob = (int)(r / d.MTc);
    const int o = ob * 32 + i, c = cb * 32 + j;
    if (o < d.Co && c < d.Ci) {
      float* q = gw + ((long long)o * d.Ci + c) * 27 + tap;
      *q = accumulate ? *q + sum : sum;
    }
  }
}

constexpr int WTH1 = 2, WTH2 = 1;  // output rows per spatial tile for stride 1 / 2

void make_wdims(WDims& d, int B, int Ci, int D, int H, int W, int Co, int stride) {
  d.B = B; d.Ci = Ci; d.Co = Co; d.D = D; d.H = H; d.W = W;
  d.Do = (D - 1) / stride + 1; d.Ho = (H - 1) / stride + 1; d.Wo = (W - 1) / stride + 1;
  d.nWt = mode::cdiv(d.Wo, 32);
  d.nHt = mode::cdiv(d.Ho, stride == 1 ? WTH1 : WTH2);
  d.T = B * d.Do * d.nHt * d.nWt;
  d.MTo = mode::cdiv(Co, 32);
  d.MTc = mode::cdiv(Ci, 32);
  int S = mode::cdiv(2 * kNumCU, d.MTo * d.MTc);
  if (S > d.T) S = d.T;
  if (S < 1) S = 1;
  d.S = S;
}

}  // namespace

namespace mode {

WgradGrid conv3d_wgrad_grid(int B, int Ci, int D, int H, int W, int Co, int stride) {
  WDims d;
  make_wdims(d, B, Ci, D, H, W, Co, stride);
  return WgradGrid{d.Do, d.Ho, d.Wo, d.nWt, d.nHt, d.MTo, d.MTc, d.S};
}

int conv3d_f32_wgrad_partials(const float* gy, const float* x, float* part, int B, int Ci, int D, int H, int W, int Co, int stride,
                              hipStream_t st, const char* who, int* S) {
  WDims d;
  make_wdims(d, B, Ci, D, H, W, Co, stride);
  *S = d.S;
  const dim3 grid(d.S, d.MTo, d.MTc);
  if (stride == 1) {
    const size_t lds = WGeom<1, WTH1>::LDS;  // same footprint: 3 planes of (WTH+2) x 34 per channel + the gy tile
    if ((long long)std::max(Ci, Co) * D * H * W >= (1ll << 29))  // (the ring kernel keeps 32-bit element offsets within a sample)
      return launch_lds(who, conv3d_bwd_weight_kernel<1, WTH1>, grid, dim3(NT), lds, st, gy, x, part, d);
    // depths per work unit: every unit starts with three un-pipelined plane loads, so as deep as the volume allows while
    // every workgroup still gets >= 2 units
    int ring_dc = ring_depths(D, (long long)B * d.nHt * d.nWt, d.S, 6);
    static const char* dc_env = getenv("MODE_RING_DC");  // (tuning override)
    if (dc_env && atoi(dc_env) > 0) ring_dc = atoi(dc_env);
    const int nDc = cdiv(D, ring_dc);
    const int units = B * d.nHt * d.nWt * nDc;
    if (d.S > units) *S = d.S = units;  // never more than the workspace query assumed
    return launch_lds(who, conv3d_bwd_weight_ring_kernel, dim3(d.S, d.MTo, d.MTc), dim3(NT), lds, st, gy, x, part, d, nDc, units, ring_dc);
  }
  const size_t lds = WGeom<2, WTH2>::LDS;
  // 32-bit element offsets within a sample of x (Ci channels at D x H x W) and of gy (Co channels at the output resolution)
  if (std::max((long long)Ci * D * H * W, (long long)Co * d.Do * d.Ho * d.Wo) >= (1ll << 29))
    return launch_lds(who, conv3d_bwd_weight_kernel<2, WTH2>, grid, dim3(NT), lds, st, gy, x, part, d);
  if (d.MTo >= 2)  // two output-channel blocks per workgroup share the staged x tile
    return launch_lds(who, conv3d_bwd_weight_s2_kernel<2>, dim3(d.S, cdiv(d.MTo, 2), d.MTc), dim3(2 * NT),
                      lds + (size_t)32 * WGeom<2, WTH2>::GPLANE * sizeof(float), st, gy, x, part, d);
  return launch_lds(who, conv3d_bwd_weight_s2_kernel<1>, grid, dim3(NT), lds, st, gy, x, part, d);
}

int conv3d_wgrad_reduce(const float* part, float* gw, int Ci, int Co, int S, int accumulate, hipStream_t st, const char* who) {
  WDims d = {};  // (reduce_gw3d reads the channel counts, their 32-blocks and the slices)
  d.Ci = Ci; d.Co = Co; d.MTo = cdiv(Co, 32); d.MTc = cdiv(Ci, 32); d.S = S;
  hipLaunchKernelGGL(reduce_gw3d, dim3(cdiv((long long)d.MTo * d.MTc * 27 * 1024, 32)), dim3(256), 0, st, part, gw, d, accumulate);
  return check_launch((std::string(who) + "(reduce)").c_str());
}

}  // namespace mode
