// 3x3x3 convolution (pad 1) for the 3D regulariser of MODE's disparity stage, gfx950 / fp32 MFMA.
//
// Reference: the stock nn.Conv3d layers inside convbn_3d (models/submodule.py:20-22) as used by dres0/dres1,
// the hourglasses and the classifiers (models/mode_disparity.py:11-46, 66-80) -- cuDNN NCDHW fp32 there.
//
// Implicit GEMM on v_mfma_f32_32x32x2_f32 with NCDHW kept as the HBM layout (W is contiguous, so one MFMA column
// tile = 32 consecutive w):
//     y[o, (d,h,w)] = sum_{tap, c} W[o, c, tap] * x[c, d+kd-1, h+kh-1, w+kw-1]        D[i = o][j = w]
//   A[i = o][k = c]   : weights, pre-packed in MFMA fragment order (one float4 = 4 channel pairs of one tap), read
//                       straight from global/L2 -- 27 KB..110 KB per layer, shared by every workgroup;
//   B[k = c][j = w]   : an input tile with halo staged in LDS, [8 channels][TD+2][TH+2][34]; lanes 0..31 of a fragment
//                       read 32 consecutive floats (conflict-free), lanes 32..63 the next channel plane.
// A workgroup (4 waves) owns TD x TH output rows of 32 voxels; each wave owns TD*TH/4 rows x all output-channel tiles.
// Input channels are streamed through LDS in chunks of 8.  Backward-data of a stride-1 convolution is the same kernel
// on gy with the weights transposed and flipped (done by the packing kernel).
//
// This file: the weight pack, the forward kernel (stride 1 | 2) and the transposed convolution with their host launchers
// (conv3d_internal.h).  The weight gradient is in conv3d_f32_wgrad.hip, the C entries are in conv3d.hip.
#include "common.h"

#include "conv3d_internal.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int NT = 256;
constexpr int CCH = 8;  // input channels per LDS chunk

struct CDims {
  int B, Ci, Co, D, H, W;  // input volume
  int Do, Ho, Wo;          // output volume: (X + 2 - 3) / stride + 1
  int nWt, nHt, nDt;       // output tiles per axis
  int MT, NCHUNK;
  int ntiles;
};

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// wp[((mt*NCHUNK + ch)*27 + tap)*64 + lane][cp] = Wsrc(o = mt*32 + (lane&31), c = ch*8 + 2*cp + (lane>>5), tap)
//   flip == 0: Wsrc(o,c,tap) = w[o][c][tap]            (forward; w is (Co,Ci,3,3,3), rows = Co, K = Ci)
//   flip == 1: Wsrc(o,c,tap) = w[c][o][26 - tap]       (backward-data: rows = Ci of the conv, K = Co)
//   flip == 2: Wsrc(o,c,tap) = w[c][o][tap]            (transposed conv: w is (Cin,Cout,3,3,3), rows = Cout, K = Cin)
//   fold != 0: row o is scaled by the folded BatchNorm scale of `bn` and block 0 writes the shifts to wp[total + o] (common.h).
__global__ void pack_w3d(const float* __restrict__ w, float* __restrict__ wp, int rows, int K, int MT, int NCHUNK, int flip,
                         int fold, mode_bn_epilogue bn) {
  const long long total = (long long)MT * NCHUNK * 27 * 64 * 4;
  if (fold && blockIdx.x == 0)
    for (int o = threadIdx.x; o < rows; o += blockDim.x) wp[total + o] = fold_shift(bn, o);
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int cp = (int)(idx & 3);
    const int lane = (int)((idx >> 2) & 63);
    long long r = idx >> 8;
    const int tap = (int)(r % 27);
    r /= 27;
    const int ch = (int)(r % NCHUNK);
    const int mt = (int)(r / NCHUNK);
    const int o = mt * 32 + (lane & 31);
    const int c = ch * CCH + 2 * cp + (lane >> 5);
    float v = 0.f;
    if (o < rows && c < K)
      v = flip == 0 ? w[((long long)o * K + c) * 27 + tap] : w[((long long)c * rows + o) * 27 + (flip == 1 ? 26 - tap : tap)];
    if (fold && o < rows) v *= fold_scale(bn, o);
    wp[idx] = v;
  }
}

// Stride 2 (S = 2): the 65 input columns of a row are stored de-interleaved, [33 odd-phase | 32 even-phase], so that the
// 32 lanes of a fragment still read consecutive LDS words: tap kw = 0 -> O[j], kw = 1 -> E[j], kw = 2 -> O[j+1].
template <int S>
__device__ __forceinline__ constexpr int tap_woff(int kw) {
  return S == 1 ? kw : (kw == 0 ? 0 : kw == 1 ? 33 : 1);
}

template <int MT, int TD, int TH, int S, bool EPI>
__global__ __launch_bounds__(NT) void conv3d_kernel(const float* __restrict__ x, const float4* __restrict__ wp,
                                                    float* __restrict__ y, CDims d, Epi epi) {
  constexpr int R = TD * TH / 4;  // output rows per wave
  constexpr int ID = (TD - 1) * S + 3, IH = (TH - 1) * S + 3;
  constexpr int IW = (S == 1) ? 34 : 65;
  constexpr int PLANE = ID * IH * IW;
  extern __shared__ __attribute__((aligned(16))) float tile[];  // [CCH][PLANE]

  // (tile order w, h, d inside an XCD's contiguous range: x is fetched 2.03 x, the depth halo of the 2-row tiles; depth-fastest
  // order was measured -- 2.26 x and the same 1.36 ms: the kernel is MFMA-bound, profiles/traffic.json)
  int t = xcd_remap(blockIdx.x, d.ntiles);
  const int wt = t % d.nWt;
  t /= d.nWt;
  const int ht = t % d.nHt;
  t /= d.nHt;
  const int dt = t % d.nDt;
  const int b = t / d.nDt;
  const int w0 = wt * 32, h0 = ht * TH, d0 = dt * TD;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const long long HW = (long long)d.H * d.W;
  const long long DHW = (long long)d.D * HW;
  const long long oHW = (long long)d.Ho * d.Wo;
  const long long oDHW = (long long)d.Do * oHW;

  f32x16 acc[MT][R];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int r = 0; r < R; ++r) acc[m][r] = (f32x16){0};

  int rowoff[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int row = wave * R + r;
    rowoff[r] = (row / TH) * S * (IH * IW) + (row % TH) * S * IW;
  }
  const float* bbase = tile + (lane >> 5) * PLANE + (lane & 31);
  const float* xb = x + (long long)b * d.Ci * DHW;

  // ---- staging of the haloed input tile, one 8-channel chunk at a time, software pipelined: the loads of chunk ch+1 are
  // issued before the MFMA phase of chunk ch and written to LDS after it.  The tile is 8 channels x RPC = ID*IH rows of IW
  // floats.  Half-wave hwv owns channel hwv of the chunk: its item j is row j / NG, 32-column group j % NG -- one coalesced
  // 128-byte load per half-wave, and (row, group) are compile-time constants, so an address is rowtab[row] + column.  The 1-2
  // remaining halo columns of every row are spread over the threads.  Loads are unconditional from clamped addresses; the
  // validity is recomputed at the LDS store (a select at the load would wait for it, or keep the masks alive across the MFMAs).
  constexpr int RPC = ID * IH;
  constexpr int NROWS = CCH * RPC;
  constexpr int NG = (S == 1) ? 1 : 2;      // 32-column groups per row
  constexpr int GO = (S == 1) ? 1 : 0;      // first column of group 0
  constexpr int NHALO = (S == 1) ? 2 : 1;   // leftover columns per row: {0, 33} or {64}
  constexpr int NIT = RPC * NG;
  constexpr int NPH = (NROWS * NHALO + NT - 1) / NT;
  static_assert(NT == 32 * CCH, "one half-wave per channel of the chunk");
  int* rowtab = reinterpret_cast<int*>(tile + CCH * PLANE);  // per row: element offset of (c, gd, gh, 0) or -1
  for (int r = tid; r < NROWS; r += NT) {
    const int c = r / RPC;
    const int rem = r - c * RPC;
    const int dz = rem / IH;
    const int hy = rem - dz * IH;
    const int gd = d0 * S + dz - 1, gh = h0 * S + hy - 1;
    rowtab[r] = (gd >= 0 && gd < d.D && gh >= 0 && gh < d.H) ? (int)(c * DHW + gd * HW + gh * d.W) : -1;
  }
  __syncthreads();
  const int hwv = tid >> 5, l32 = tid & 31;
  const int* myrows = rowtab + hwv * RPC;
  float* mytile = tile + hwv * PLANE;
  float vm[NIT], vh[NPH];

  auto issue = [&](int ch) {
    const float* xc = xb + (long long)ch * CCH * DHW;
    const bool cok = ch * CCH + hwv < d.Ci;
#pragma unroll
    for (int j = 0; j < NIT; ++j) {
      const int rem = j / NG, g = j % NG;
      const int gw = w0 * S + GO + 32 * g + l32 - 1;
      const int off = myrows[rem];
      const bool ok = cok && off >= 0 && gw >= 0 && gw < d.W;
      vm[j] = xc[(unsigned)(ok ? off + gw : 0)];
    }
#pragma unroll
    for (int k = 0; k < NPH; ++k) {
      const int item = k * NT + tid;
      const int r = item / NHALO, side = item - r * NHALO;
      const int wx = (S == 1) ? (side ? 33 : 0) : 64;
      const int gw = w0 * S + wx - 1;
      const int off = (item < NROWS * NHALO) ? rowtab[r] : -1;
      const bool ok = off >= 0 && gw >= 0 && gw < d.W && ch * CCH + r / RPC < d.Ci;
      vh[k] = xc[(unsigned)(ok ? off + gw : 0)];
    }
  };
  auto commit = [&](int ch) {
    const bool cok = ch * CCH + hwv < d.Ci;
#pragma unroll
    for (int j = 0; j < NIT; ++j) {
      const int rem = j / NG, g = j % NG;
      const int wx = GO + 32 * g + l32;
      const int gw = w0 * S + wx - 1;
      const int lw = (S == 1) ? wx : ((wx & 1) ? 33 + (wx >> 1) : (wx >> 1));
      const bool ok = cok && myrows[rem] >= 0 && gw >= 0 && gw < d.W;
      mytile[rem * IW + lw] = ok ? vm[j] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < NPH; ++k) {
      const int item = k * NT + tid;
      const int r = item / NHALO, side = item - r * NHALO;
      const int wx = (S == 1) ? (side ? 33 : 0) : 64;
      const int gw = w0 * S + wx - 1;
      const int lw = (S == 1) ? wx : 32;  // column 64 = odd-phase entry O[32] of the [O | E] split
      if (item < NROWS * NHALO) {
        const bool ok = rowtab[r] >= 0 && gw >= 0 && gw < d.W && ch * CCH + r / RPC < d.Ci;
        tile[r * IW + lw] = ok ? vh[k] : 0.f;
      }
    }
  };

  issue(0);
  commit(0);
  __syncthreads();
  for (int ch = 0; ch < d.NCHUNK; ++ch) {
    if (ch + 1 < d.NCHUNK) {
      issue(ch + 1);  // in flight during the MFMA phase below
      __builtin_amdgcn_sched_barrier(0);
    }
    // ---- 27 taps x 4 channel pairs x R rows x MT tiles of MFMA
    // weights one tap ahead: the fragment of tap t+1 is requested half-way through the MFMAs of tap t (the compiler on its
    // own requested it right before its first use and waited a full L1/L2 round trip every other tap)
    const float4* wq = wp + ((long long)ch * 27) * 64 + lane;
    float4 a_nxt[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) a_nxt[m] = wq[((long long)m * d.NCHUNK * 27) * 64];
#pragma unroll
    for (int tap = 0; tap < 27; ++tap) {
      const int toff = (tap / 9) * (IH * IW) + ((tap / 3) % 3) * IW + tap_woff<S>(tap % 3);
      float4 a4[MT];
#pragma unroll
      for (int m = 0; m < MT; ++m) a4[m] = a_nxt[m];
#pragma unroll
      for (int cp = 0; cp < 4; ++cp) {
        if (cp == 2) {
          if (tap + 1 < 27) {
#pragma unroll
            for (int m = 0; m < MT; ++m) a_nxt[m] = wq[((long long)m * d.NCHUNK * 27 + tap + 1) * 64];
          }
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const float bv = bbase[2 * cp * PLANE + toff + rowoff[r]];
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            const float av = cp == 0 ? a4[m].x : cp == 1 ? a4[m].y : cp == 2 ? a4[m].z : a4[m].w;
            acc[m][r] = mfma32(av, bv, acc[m][r]);
          }
        }
      }
    }
    __syncthreads();  // every wave is done reading this chunk
    if (ch + 1 < d.NCHUNK) {
      commit(ch + 1);
      __syncthreads();
    }
  }

  // ---- epilogue: D[i = o][j = w]
  float* yb = y + (long long)b * d.Co * oDHW;
  const int gw = w0 + (lane & 31);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int row = wave * R + r;
    const int gd = d0 + row / TH, gh = h0 + row % TH;
    if (gd < d.Do && gh < d.Ho && gw < d.Wo) {
      const long long sp = gd * oHW + (long long)gh * d.Wo + gw;
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int o = m * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
          if (o < d.Co) {
            const long long idx = o * oDHW + sp;
            yb[idx] = EPI ? apply_epi(epi, acc[m][r][q], o, (long long)b * d.Co * oDHW + idx) : acc[m][r][q];
          }
        }
    }
  }
}

template <int MT, int TD, int TH, int S>
int launch_conv(const float* x, const float* wpack, float* y, CDims d, hipStream_t st, const char* who, Epi epi) {
  d.nWt = mode::cdiv(d.Wo, 32);
  d.nHt = mode::cdiv(d.Ho, TH);
  d.nDt = mode::cdiv(d.Do, TD);
  d.ntiles = d.B * d.nDt * d.nHt * d.nWt;
  constexpr int kRows = CCH * ((TD - 1) * S + 3) * ((TH - 1) * S + 3);
  const size_t lds = (size_t)kRows * (S == 1 ? 34 : 65) * sizeof(float) + (size_t)kRows * sizeof(int);  // tile + row table
  // (an eval-mode layer with the folded BatchNorm epilogue has its own instantiation, the plain kernel is untouched)
  return mode::launch_lds(who, epi.shift ? conv3d_kernel<MT, TD, TH, S, true> : conv3d_kernel<MT, TD, TH, S, false>, dim3(d.ntiles),
                          dim3(NT), lds, st, x, reinterpret_cast<const float4*>(wpack), y, d, epi);
}

// What the three launchers below start with: d for a GEMM of `rows` output channels over K reduction channels, x (B, K, D, H, W) ->
// (B, rows, Do, Ho, Wo) (the tile counts are the launcher's); the weights packed behind `flip` (pack_w3d) unless the caller's pack is
// kept, with the BatchNorm of `bn` folded in; the epilogue that reads the folded shifts behind the pack.
Epi conv_setup(CDims& d, const float* w, float* wpack, int B, int K, int rows, int D, int H, int W, int Do, int Ho, int Wo, int flip,
               const mode_bn_epilogue* bn, hipStream_t st) {
  d.B = B; d.Ci = K; d.Co = rows; d.D = D; d.H = H; d.W = W;
  d.Do = Do; d.Ho = Ho; d.Wo = Wo;
  d.MT = mode::cdiv(rows, 32);
  d.NCHUNK = mode::cdiv(K, CCH);
  const long long npack = (long long)mode::conv3d_f32_pack_floats(K, rows);
  if (mode::pack_needed()) hipLaunchKernelGGL(pack_w3d, dim3(mode::cdiv(npack, 256)), dim3(256), 0, st, w, wpack, rows, K, d.MT, d.NCHUNK, flip, bn ? 1 : 0,
                     bn ? *bn : mode_bn_epilogue());
  return make_epi(bn, wpack + npack);
}

// ---------------------------------------------------------------------------------------------------------------------
// Transposed convolution k3 s2 p1 op1 (ConvTranspose3d of hourglass conv5/conv6, mode_disparity.py:23, 25) = the
// backward-data of the stride-2 convolution:   out[o, z] = sum_{c, k : z = 2q - 1 + k} Wsrc(o, c, k) * x[c, q],  out = 2 x in.
// Split by output parity per axis: an even output coordinate z = 2q' uses only k = 1 (q = q'); an odd one z = 2q'+1 uses
// k = 2 (q = q') and k = 0 (q = q'+1).  The 8 parity classes of one low-resolution voxel carry 1+2+2+2+4+4+4+8 = 27
// taps, so no MFMA is spent on structural zeros.  D[i = o][j = 32 low-res w]; a wave owns one low-res row and keeps the
// 8 class accumulators live; the two w-parities of a row are stored interleaved as one float2 per lane (coalesced).
// Weight tap (kd*9 + kh*3 + kw) of the n-th MFMA group of deconv3d_kernel, in the order its parity-class loops run.
__host__ __device__ constexpr int deconv_wtap(int n) {
  int i = 0;
  for (int pd = 0; pd < 2; ++pd)
    for (int ph = 0; ph < 2; ++ph)
      for (int pw = 0; pw < 2; ++pw)
        for (int td = 0; td <= pd; ++td)
          for (int th = 0; th <= ph; ++th)
            for (int tw = 0; tw <= pw; ++tw) {
              if (i == n) return (pd ? (td ? 0 : 2) : 1) * 9 + (ph ? (th ? 0 : 2) : 1) * 3 + (pw ? (tw ? 0 : 2) : 1);
              ++i;
            }
  return 0;
}

template <int TD, int TH, bool EPI>
__global__ __launch_bounds__(NT, EPI ? 2 : 1) void deconv3d_kernel(const float* __restrict__ x, const float4* __restrict__ wp,
                                                      float* __restrict__ y, CDims d, Epi epi) {
  static_assert(TD * TH == 4, "one low-resolution row per wave");
  constexpr int ID = TD + 1, IH = TH + 1, IW = 33;
  constexpr int PLANE = ID * IH * IW;
  extern __shared__ __attribute__((aligned(16))) float tile[];  // [CCH][PLANE]

  int t = xcd_remap(blockIdx.x, d.ntiles);
  const int wt = t % d.nWt;
  t /= d.nWt;
  const int ht = t % d.nHt;
  t /= d.nHt;
  const int dt = t % d.nDt;
  const int b = t / d.nDt;
  const int mt = blockIdx.y;
  const int w0 = wt * 32, h0 = ht * TH, d0 = dt * TD;  // low-resolution (input) coordinates
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const long long HW = (long long)d.H * d.W;
  const long long DHW = (long long)d.D * HW;
  const long long oHW = (long long)d.Ho * d.Wo;
  const long long oDHW = (long long)d.Do * oHW;

  f32x16 acc[2][2][2];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i >> 2][(i >> 1) & 1][i & 1] = (f32x16){0};

  const int dz = wave / TH, hy = wave % TH;
  const float* bbase = tile + (lane >> 5) * PLANE + dz * (IH * IW) + hy * IW + (lane & 31);
  const float* xb = x + (long long)b * d.Ci * DHW;

  // Staging, software pipelined like conv3d_kernel: half-wave hwv owns channel hwv of the 8-channel chunk; its item j is tile
  // row j (RPC = ID*IH rows of 32 coalesced columns), the 33rd column of every row is one more load for the first 72 threads.
  // The loads of chunk ch+1 are issued before the MFMAs of chunk ch and written to LDS after them.
  constexpr int RPC = ID * IH, NROWS = CCH * RPC;
  static_assert(NROWS <= NT, "one thread per row for the leftover column");
  const int hwv = tid >> 5, l32 = tid & 31;
  int rowoff[RPC];
  unsigned rowok = 0;
#pragma unroll
  for (int j = 0; j < RPC; ++j) {
    const int gd = d0 + j / IH, gh = h0 + j % IH;
    const bool ok = gd < d.D && gh < d.H && w0 + l32 < d.W;
    rowoff[j] = ok ? (int)(gd * HW + gh * d.W) + w0 + l32 : 0;
    rowok |= (ok ? 1u : 0u) << j;
  }
  const int e_c = tid / RPC, e_rem = tid - e_c * RPC;  // leftover-column item of thread tid < NROWS
  const int e_gd = d0 + e_rem / IH, e_gh = h0 + e_rem % IH;
  const bool e_in = tid < NROWS && e_gd < d.D && e_gh < d.H && w0 + 32 < d.W;
  const int e_off = e_in ? (int)(e_gd * HW + e_gh * d.W) + w0 + 32 : 0;
  float vm[RPC], ve;
  auto issue = [&](int ch) {
    const bool cok = ch * CCH + hwv < d.Ci;
    // (a half-wave whose channel lies beyond Ci reads the chunk's FIRST channel instead -- the value is dropped in commit().  Round 6:
    // the base used to include the missing channel itself, i.e. an address up to 7 planes past the end of the last sample -- harmless
    // inside a cached allocation, a memory fault when x ended at the end of a mapping: the full GPU suite hit it once its order changed)
    const float* xc = xb + ((long long)ch * CCH + (cok ? hwv : 0)) * DHW;
#pragma unroll
    for (int j = 0; j < RPC; ++j) vm[j] = xc[(unsigned)(cok ? rowoff[j] : 0)];
    const bool eok = e_in && ch * CCH + e_c < d.Ci;
    ve = xb[eok ? ((long long)ch * CCH + e_c) * DHW + e_off : 0];
  };
  auto commit = [&](int ch) {
    const bool cok = ch * CCH + hwv < d.Ci;
    float* dst = tile + hwv * PLANE + l32;
#pragma unroll
    for (int j = 0; j < RPC; ++j) dst[j * IW] = (cok && ((rowok >> j) & 1)) ? vm[j] : 0.f;
    if (tid < NROWS) tile[tid * IW + 32] = (e_in && ch * CCH + e_c < d.Ci) ? ve : 0.f;
  };

  issue(0);
  commit(0);
  __syncthreads();
  for (int ch = 0; ch < d.NCHUNK; ++ch) {
    if (ch + 1 < d.NCHUNK) {
      issue(ch + 1);
      __builtin_amdgcn_sched_barrier(0);
    }
    // The 27 taps touch only 8 distinct input voxels per channel pair ((dq_d, dq_h, dq_w) in {0,1}^3): the 32 B operands of the
    // chunk are read from LDS once, up front.  The weight fragment of tap n+2 is requested while tap n runs (the compiler on
    // its own requested every fragment right before its first use and waited for the L1/L2 round trip).
    const float4* wq = wp + (((long long)mt * d.NCHUNK + ch) * 27) * 64 + lane;
    float bop[4][8];
#pragma unroll
    for (int cp = 0; cp < 4; ++cp)
#pragma unroll
      for (int v = 0; v < 8; ++v) bop[cp][v] = bbase[2 * cp * PLANE + (v >> 2) * (IH * IW) + ((v >> 1) & 1) * IW + (v & 1)];
    float4 w_a = wq[deconv_wtap(0) * 64], w_b = wq[deconv_wtap(1) * 64];
    int n = 0;
#pragma unroll
    for (int pd = 0; pd < 2; ++pd)
#pragma unroll
      for (int ph = 0; ph < 2; ++ph)
#pragma unroll
        for (int pw = 0; pw < 2; ++pw)
#pragma unroll
          for (int td = 0; td <= pd; ++td)
#pragma unroll
            for (int th = 0; th <= ph; ++th)
#pragma unroll
              for (int tw = 0; tw <= pw; ++tw) {
                // parity 0: (k = 1, dq = 0); parity 1: t = 0 -> (k = 2, dq = 0), t = 1 -> (k = 0, dq = 1)
                const int v = ((pd ? td : 0) << 2) | ((ph ? th : 0) << 1) | (pw ? tw : 0);
                const float4 a4 = w_a;
                w_a = w_b;
                if (n + 2 < 27) w_b = wq[deconv_wtap(n + 2) * 64];
                ++n;
                __builtin_amdgcn_sched_barrier(0);
                acc[pd][ph][pw] = mfma32(a4.x, bop[0][v], acc[pd][ph][pw]);
                acc[pd][ph][pw] = mfma32(a4.y, bop[1][v], acc[pd][ph][pw]);
                acc[pd][ph][pw] = mfma32(a4.z, bop[2][v], acc[pd][ph][pw]);
                acc[pd][ph][pw] = mfma32(a4.w, bop[3][v], acc[pd][ph][pw]);
              }
    __syncthreads();
    if (ch + 1 < d.NCHUNK) {
      commit(ch + 1);
      __syncthreads();
    }
  }

  float* yb = y + (long long)b * d.Co * oDHW;
  const int qd = d0 + dz, qh = h0 + hy, qw = w0 + (lane & 31);
  // the folded-BatchNorm shifts of this lane's 16 output channels, once: read inside the store loop (`epi.shift` may alias y as far as
  // the compiler knows) every store waited for a load of its own -- 64 serialised L2 round trips per lane and tile (round 5, ISA scan)
  float shv[16];
  if (EPI) {
#pragma unroll
    for (int q = 0; q < 16; ++q) shv[q] = epi.shift[min(mt * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5), d.Co - 1)];
  }
  if (qd < d.D && qh < d.H && qw < d.W) {
#pragma unroll
    for (int pd = 0; pd < 2; ++pd)
#pragma unroll
      for (int ph = 0; ph < 2; ++ph) {
        const long long sp = (long long)(2 * qd + pd) * oHW + (long long)(2 * qh + ph) * d.Wo + 2 * qw;
        // the residual of this (pd, ph) row: its 16 float2 loads are issued together BEFORE the row's stores.  Read next to the
        // stores (`add` may alias `y` as far as the compiler knows) every load waited for the store in front of it: 0.43 ms for the
        // 64 -> 32 layer of one pair against 0.24 without the residual, whose 201 MB are 0.04 ms of traffic.
        float2 res[16];
        if (EPI) {
#pragma unroll
          for (int q = 0; q < 16; ++q) res[q] = make_float2(0.f, 0.f);
          if (epi.add) {  // (one uniform test around the 16 loads, not one per load)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
              const int o = min(mt * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5), d.Co - 1);
              res[q] = *reinterpret_cast<const float2*>(epi.add + (long long)b * d.Co * oDHW + o * oDHW + sp);
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        auto emit = [&](int q) {
          const int o = mt * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
          float2 v = make_float2(acc[pd][ph][0][q], acc[pd][ph][1][q]);
          if (EPI) {  // torch's order: (convolution * scale + shift) + residual, then ReLU
            const float sh = shv[q];
            v = make_float2((v.x + sh) + res[q].x, (v.y + sh) + res[q].y);
            if (epi.relu) v = make_float2(relu_nan(v.x), relu_nan(v.y));
          }
          *reinterpret_cast<float2*>(yb + o * oDHW + sp) = v;
        };
        if (mt * 32 + 32 <= d.Co) {  // a full tile of output channels (uniform): 16 stores in one block -- with a test per channel every
#pragma unroll                        // store was its own basic block behind a vmcnt(0), i.e. behind the store in front of it
          for (int q = 0; q < 16; ++q) emit(q);
        } else {
#pragma unroll
          for (int q = 0; q < 16; ++q)
            if (mt * 32 + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5) < d.Co) emit(q);
        }
        if (EPI) __builtin_amdgcn_sched_barrier(0);
      }
  }
}

}  // namespace

// ---- the host launchers (conv3d_internal.h)
namespace mode {

size_t conv3d_f32_pack_floats(int K, int rows) { return (size_t)cdiv(rows, 32) * cdiv(K, CCH) * 27 * 256; }

int conv3d_s1(const float* x, const float* w, float* y, float* wpack, int B, int K, int rows, int D, int H, int W, int flip,
              hipStream_t st, const char* who, const mode_bn_epilogue* bn) {
  MODE_REQUIRE(rows <= 64, MODE_ERR_UNSUPPORTED, "%s: more than 64 output channels (%d) not supported", who, rows);
  CDims d;
  const Epi epi = conv_setup(d, w, wpack, B, K, rows, D, H, W, D, H, W, flip, bn, st);
  // tile choice: keep >= 2 workgroups per CU worth of tiles if possible
  const long long big = (long long)B * cdiv(D, 2) * cdiv(H, 8) * cdiv(W, 32);
  const long long mid = (long long)B * cdiv(D, 2) * cdiv(H, 4) * cdiv(W, 32);
  if (d.MT == 1) {
    if (big >= 2 * kNumCU) return launch_conv<1, 2, 8, 1>(x, wpack, y, d, st, who, epi);
    if (mid >= 2 * kNumCU) return launch_conv<1, 2, 4, 1>(x, wpack, y, d, st, who, epi);
    return launch_conv<1, 1, 4, 1>(x, wpack, y, d, st, who, epi);
  }
  // (the 2x8 tile with two output-channel tiles needs 268 registers -> one wave per SIMD; 2x4 keeps two)
  if (mid >= 2 * kNumCU) return launch_conv<2, 2, 4, 1>(x, wpack, y, d, st, who, epi);
  return launch_conv<2, 1, 4, 1>(x, wpack, y, d, st, who, epi);
}

int conv3d_s2(const float* x, const float* w, float* y, float* wpack, int B, int K, int rows, int D, int H, int W, hipStream_t st,
              const char* who, const mode_bn_epilogue* bn) {
  MODE_REQUIRE(rows <= 64, MODE_ERR_UNSUPPORTED, "%s: more than 64 output channels (%d) not supported", who, rows);
  CDims d;
  const Epi epi = conv_setup(d, w, wpack, B, K, rows, D, H, W, (D - 1) / 2 + 1, (H - 1) / 2 + 1, (W - 1) / 2 + 1, 0, bn, st);
  if (d.MT == 1) return launch_conv<1, 1, 4, 2>(x, wpack, y, d, st, who, epi);
  return launch_conv<2, 1, 4, 2>(x, wpack, y, d, st, who, epi);
}

// (the weights are packed with flip 2 -- see pack_w3d -- for ConvTranspose3d weights and for the backward-data of a stride-2 Conv3d)
int deconv3d(const float* x, const float* w, float* y, float* wpack, int B, int K, int rows, int D, int H, int W, hipStream_t st,
             const char* who, const mode_bn_epilogue* bn) {
  CDims d;
  const Epi epi = conv_setup(d, w, wpack, B, K, rows, D, H, W, 2 * D, 2 * H, 2 * W, 2, bn, st);
  constexpr int TD = 2, TH = 2;
  d.nWt = cdiv(W, 32);
  d.nHt = cdiv(H, TH);
  d.nDt = cdiv(D, TD);
  d.ntiles = B * d.nDt * d.nHt * d.nWt;
  const size_t lds = (size_t)CCH * (TD + 1) * (TH + 1) * 33 * sizeof(float);  // (below the 64 KiB that need the opt-in)
  return launch_lds(who, epi.shift ? deconv3d_kernel<TD, TH, true> : deconv3d_kernel<TD, TH, false>, dim3(d.ntiles, d.MT), dim3(NT), lds,
                    st, x, reinterpret_cast<const float4*>(wpack), y, d, epi);
}

}  // namespace mode
