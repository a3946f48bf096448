// Spherical convolution, "windowed" forward kernels for gfx950 (MI355X): the fp32 tiles of every window class, and the small- and
// tall-window tiles on the split arithmetic of split_arith.h.  sphere_win_internal.h says what a window is and who plans the tiles.
//
// The general kernels of sphere_conv.hip gather the four bilinear corners of every (channel, tap, pixel) sample straight from
// global memory: 4 dependent loads and ~50 VALU instructions per sample, which bound them at 22-44 % of the fp32 MFMA peak.
// These kernels stage the window of the input ONCE per channel chunk in LDS with plain row loads and build the MFMA B operand
// on the fly from it: 4 LDS reads + 4 FMAs per sample, no column buffer at all.
//
// Tile = 32 rows x 4 columns of output pixels (stride 1): wave v owns column w0 + v and the 32 rows h0 .. h0+31 as the N
// dimension of v_mfma_f32_32x32x2_f32 (lanes run along h: for the Cassini layout of the network that is the longitude axis,
// so the 32 lanes of a half-wave read 32 consecutive LDS words), and all (<= 128) output channels of its z-slice as 4 M-tiles.
// K is ordered chunk (8 input channels) > tap > channel pair; the two half-waves supply the two channels of a pair.
//
// Reference: sphere_conv_cuda_kernel.cu:83-113, 195-262 (im2col gather) + sphere_conv_cuda.cpp:177-205 (addmm_).
#include "sphere_win_internal.h"

namespace {

// wp[(((g*MG + mg)*NCH + ch)*KT + tap)*MTW + m][lane] (float4 = 4 k-steps) = W[g*Cog + mg*128 + m*32 + (lane&31)][ch*8 + 2*s + (lane>>5)][tap]
//   fold != 0: output channel co is scaled by the folded BatchNorm scale of `bn`; block 0 writes the shifts to wp[total + channel]
__global__ void pack_w_win(const float* __restrict__ w, float* __restrict__ wp, WinDims d, int fold, mode_bn_epilogue bn) {
  const long long total = (long long)d.G * d.MG * d.NCH * KT * MTW * 64 * 4;
  if (fold && blockIdx.x == 0)
    for (int o = threadIdx.x; o < d.Co; o += blockDim.x) wp[total + o] = fold_shift(bn, o);
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    const int s = (int)(idx & 3);
    const int lane = (int)((idx >> 2) & 63);
    long long r = idx >> 8;
    const int m = (int)(r % MTW);
    r /= MTW;
    const int tap = (int)(r % KT);
    r /= KT;
    const int ch = (int)(r % d.NCH);
    r /= d.NCH;
    const int mg = (int)(r % d.MG);
    const int g = (int)(r / d.MG);
    const int co = mg * 128 + m * 32 + (lane & 31);
    const int c = ch * CCH + 2 * s + (lane >> 5);
    float v = 0.f;
    if (co < d.Cog && c < d.Cig) {
      v = w[((long long)(g * d.Cog + co) * d.Cig + c) * KT + tap];
      if (fold) v *= fold_scale(bn, g * d.Cog + co);
    }
    wp[idx] = v;
  }
}

// One tile.  WR_T > 0: compile-time window rows; WR_T == 0: window rows = d.wr (wrap-around class).  PIPE: double-buffered,
// the next chunk's rows are prefetched into registers under the MFMA phase, in NPH phases of CCH/NPH channels each (a tall
// window has too many rows to hold a whole chunk in registers); otherwise single buffer, staged in place.
template <int WR_T, bool PIPE, int NRB, int NPH, bool EPI>
__device__ __forceinline__ void fwd_tile(const float* __restrict__ x, const float* __restrict__ pos, const float4* __restrict__ wp,
                                         float* __restrict__ y, const WinDims& d, int h0, int w0, int rbase, int cbase, float* smem,
                                         const Epi& epi) {
  const int WRP = WR_T > 0 ? WR_T : d.wr;
  const int CP = chan_pitch(WRP);
  const int bufsz = CCH * CP;

  const int b = blockIdx.y;
  const int g = blockIdx.z / d.MG, mg = blockIdx.z % d.MG;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int half = lane >> 5;
  const int h = h0 + (wave / TW) * 32 + (lane & 31), w = w0 + (wave % TW);
  const bool pix_ok = h < d.H && w < d.W;
  const long long HW = (long long)d.H * d.W;

  // sampling records of this lane's pixel: window offset of the first corner + 4 weights per tap, kept in registers
  int roff[KT];
  float4 rw[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    int r0 = 0, c0 = 0;
    float4 wt = make_float4(0.f, 0.f, 0.f, 0.f);
    if (pix_ok) {
      const long long idx = (long long)h * d.W + w;
      mode::tap_record_fixed(pos[(2 * k) * HW + idx], pos[(2 * k + 1) * HW + idx], d.H, d.W, r0, c0, wt);
    }
    int lr = r0 - rbase;
    if (lr < 0) lr += d.H;
    const int lc = c0 - cbase;
    const bool dead = wt.x == 0.f && wt.y == 0.f && wt.z == 0.f && wt.w == 0.f;
    roff[k] = (dead || !pix_ok) ? 0 : lc * WRP + lr;
    rw[k] = wt;
  }

  // every LDS word that can be read must be finite: zero everything once (corners with weight 0 may point anywhere inside)
  const int lds_floats = (PIPE ? 2 : 1) * bufsz + WRP + 8;
  for (int i = tid; i < lds_floats; i += NTHREADS) smem[i] = 0.f;
  __syncthreads();

  // staging: thread -> (window column, row within a pass of SROWS rows)
  // lanes run along the contiguous axis of the planes: columns for NCHW, rows when the planes are stored transposed
  const int scol = d.sh == 1 ? tid / SROWS : tid & (WC - 1), srow = d.sh == 1 ? tid % SROWS : tid / WC;
  const int gcol = cbase + scol;
  const bool col_ok = gcol < d.W;
  const float* xg = x + ((long long)b * d.Ci + (long long)g * d.Cig) * HW + (col_ok ? gcol * d.sw : 0);
  int rowoff[NRB];  // global offset of the source row of each pass (rows wrap around the axis; H*W < 2^30)
#pragma unroll
  for (int rb = 0; rb < NRB; ++rb) {
    const int r = rb * SROWS + srow;
    rowoff[rb] = ((rbase + (r < WRP ? r : 0)) % d.H) * d.sh;
  }
  constexpr int CPH = CCH / NPH;  // channels per staging phase
  float lv[PIPE ? CPH * NRB : 1];

  auto issue = [&](int ch, int ph) {
#pragma unroll
    for (int cc = 0; cc < CPH; ++cc) {
      const int chan = ch * CCH + ph * CPH + cc;
      const float* xc = xg + (long long)(chan < d.Cig ? chan : 0) * HW;
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb) lv[cc * NRB + rb] = xc[rowoff[rb]];
    }
  };
  auto commit = [&](int ch, int ph, float* buf) {
#pragma unroll
    for (int cc = 0; cc < CPH; ++cc) {
      const int c = ph * CPH + cc;
      const bool ok = col_ok && (ch * CCH + c < d.Cig);
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb) {
        const int r = rb * SROWS + srow;
        if (r < WRP) buf[c * CP + scol * WRP + r] = ok ? lv[cc * NRB + rb] : 0.f;
      }
    }
  };
  auto stage_now = [&](int ch, float* buf) {  // tall windows: plain loop, 4 loads in flight per thread
    for (int r = srow; r < WRP; r += SROWS) {
      const int ro = ((rbase + r) % d.H) * d.sh;
#pragma unroll
      for (int c4 = 0; c4 < CCH; c4 += 4) {
        float t4[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int chan = ch * CCH + c4 + c;
          t4[c] = xg[(long long)(chan < d.Cig ? chan : 0) * HW + ro];
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) buf[(c4 + c) * CP + scol * WRP + r] = (col_ok && ch * CCH + c4 + c < d.Cig) ? t4[c] : 0.f;
      }
    }
  };

  f32x16 acc[MTW];
#pragma unroll
  for (int m = 0; m < MTW; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;

  const float4* wpa = wp + ((long long)(g * d.MG + mg) * d.NCH) * KT * MTW * 64 + lane;
  const int nsteps = d.NCH * KT;
  float4 a_cur[MTW], a_nxt[MTW];
#pragma unroll
  for (int m = 0; m < MTW; ++m) a_cur[m] = wpa[m * 64];

  // B operand of tap k for the 4 channel pairs of the chunk in `buf`: 4 LDS reads (load_raw) + 4 FMAs (combine, operand
  // order of cu:111) each.  The two halves are separate so that the reads of the NEXT tap can be issued before the MFMAs of
  // the current one and combined after them; the scheduling barriers keep the compiler from sinking the prefetches (weights
  // from L2, window words from LDS) down to their first use, which would expose their latency on every tap.
  auto load_raw = [&](const float* buf, int k, float (&raw)[16]) {
    const float* p = buf + half * CP + roff[k];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const float* q = p + 2 * s * CP;
      raw[s * 4 + 0] = q[0];
      raw[s * 4 + 1] = q[WRP];
      raw[s * 4 + 2] = q[1];
      raw[s * 4 + 3] = q[WRP + 1];
    }
  };
  auto combine = [&](const float (&raw)[16], int k, float (&v)[4]) {
    const float4 tw = rw[k];
#pragma unroll
    for (int s = 0; s < 4; ++s) v[s] = tw.x * raw[s * 4] + tw.y * raw[s * 4 + 1] + tw.z * raw[s * 4 + 2] + tw.w * raw[s * 4 + 3];
  };

  if (PIPE) {
#pragma unroll
    for (int ph = 0; ph < NPH; ++ph) {
      issue(0, ph);
      commit(0, ph, smem);
    }
    __syncthreads();
  }
  constexpr int TPP = KT / NPH;  // taps per staging phase (the last phase also takes the remainder)
  for (int ch = 0; ch < d.NCH; ++ch) {
    float* cur = smem + (PIPE ? (ch & 1) * bufsz : 0);
    float* nxt = smem + (PIPE ? ((ch + 1) & 1) * bufsz : 0);
    const bool more = ch + 1 < d.NCH;
    if (!PIPE) {
      if (ch > 0) __syncthreads();  // everyone is done reading the previous chunk
      stage_now(ch, cur);
      __syncthreads();
    }
    float vb[4], raw[16];
    load_raw(cur, 0, raw);
    combine(raw, 0, vb);
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      const int step = ch * KT + k;
      const int nstep = step + 1 < nsteps ? step + 1 : step;
      if (PIPE && k % TPP == 0 && k / TPP < NPH && more) issue(ch + 1, k / TPP);  // rows of the next chunk fly under the MFMAs below
#pragma unroll
      for (int m = 0; m < MTW; ++m) a_nxt[m] = wpa[((long long)nstep * MTW + m) * 64];
      if (k + 1 < KT) load_raw(cur, k + 1, raw);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float a0 = s == 0 ? a_cur[0].x : s == 1 ? a_cur[0].y : s == 2 ? a_cur[0].z : a_cur[0].w;
        const float a1 = s == 0 ? a_cur[1].x : s == 1 ? a_cur[1].y : s == 2 ? a_cur[1].z : a_cur[1].w;
        const float a2 = s == 0 ? a_cur[2].x : s == 1 ? a_cur[2].y : s == 2 ? a_cur[2].z : a_cur[2].w;
        const float a3 = s == 0 ? a_cur[3].x : s == 1 ? a_cur[3].y : s == 2 ? a_cur[3].z : a_cur[3].w;
        acc[0] = mfma32(a0, vb[s], acc[0]);
        acc[1] = mfma32(a1, vb[s], acc[1]);
        acc[2] = mfma32(a2, vb[s], acc[2]);
        acc[3] = mfma32(a3, vb[s], acc[3]);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (k + 1 < KT) combine(raw, k + 1, vb);
#pragma unroll
      for (int m = 0; m < MTW; ++m) a_cur[m] = a_nxt[m];
      if (PIPE && more && (k == KT - 1 || (k % TPP == TPP - 1 && k / TPP < NPH - 1)))
        commit(ch + 1, k == KT - 1 ? NPH - 1 : k / TPP, nxt);  // the other buffer: nobody reads it now
    }
    if (PIPE) __syncthreads();
  }

  if (pix_ok) {
    float* yb = y + ((long long)b * d.Co + (long long)g * d.Cog + (long long)mg * 128) * HW + (long long)h * d.sh + (long long)w * d.sw;
    const int cmax = d.Cog - mg * 128;
#pragma unroll
    for (int m = 0; m < MTW; ++m) {
      // eval mode: the shifts and the residual of this output tile, requested together ahead of its stores (see sphere_fwd_split_kernel)
      float res[16], shv[16];
      if (EPI) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int co = min(MODE_ACC_ROW(m, r, half), cmax - 1);
          shv[r] = epi.shift[g * d.Cog + mg * 128 + co];
          res[r] = 0.f;
        }
        if (epi.add) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int co = min(MODE_ACC_ROW(m, r, half), cmax - 1);
            res[r] = epi.add[(yb - y) + (long long)co * HW];
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      auto emit = [&](int r) {
        const int co = MODE_ACC_ROW(m, r, half);
        if (EPI) {  // folded BatchNorm shift (+ residual) (+ ReLU) on the way out
          const float v = (acc[m][r] + shv[r]) + res[r];
          yb[(long long)co * HW] = epi.relu ? relu_nan(v) : v;
        } else {
          yb[(long long)co * HW] = acc[m][r];
        }
      };
      if (m * 32 + 32 <= cmax) {
#pragma unroll
        for (int r = 0; r < 16; ++r) emit(r);
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (MODE_ACC_ROW(m, r, half) < cmax) emit(r);
      }
      if (EPI) __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// grid = (tiles, B, G*MG); tiles[i] = (h0, w0, rbase, cbase | class << 16).  All window classes run in ONE launch so that
// the few tall-window tiles next to the poles overlap with the rest instead of forming an under-filled tail of their own.
template <bool EPI>
__global__ __launch_bounds__(NTHREADS) void sphere_fwd_win_kernel(const float* __restrict__ x, const float* __restrict__ pos,
                                                                   const float4* __restrict__ wp, float* __restrict__ y, WinDims d,
                                                                   const int4* __restrict__ tiles, Epi epi) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int4 t = tiles[blockIdx.x];  // (list order = tall-window tiles first; an XCD-contiguous order would pile them on one XCD)
  const int cls = t.w >> 16, cbase = t.w & 0xffff;
  if (cls == 0)
    fwd_tile<WR_SMALL, true, (WR_SMALL + SROWS - 1) / SROWS, 1, EPI>(x, pos, wp, y, d, t.x, t.y, t.z, cbase, smem, epi);
  else if (cls == 1)
    fwd_tile<WR_MID, true, (WR_MID + SROWS - 1) / SROWS, 2, EPI>(x, pos, wp, y, d, t.x, t.y, t.z, cbase, smem, epi);
  else
    fwd_tile<0, true, WR_PIPE_MAX / SROWS, 4, EPI>(x, pos, wp, y, d, t.x, t.y, t.z, cbase, smem, epi);
}

// Wrap-around tiles of images too tall for the double-buffered form (H + 1 > 320 rows, or more LDS than there is): single
// buffer, staged in place.  A kernel of its own so that its register needs do not weigh on the main one.
template <bool EPI>
__global__ __launch_bounds__(NTHREADS) void sphere_fwd_win_tall_kernel(const float* __restrict__ x, const float* __restrict__ pos,
                                                                        const float4* __restrict__ wp, float* __restrict__ y,
                                                                        WinDims d, const int4* __restrict__ tiles, Epi epi) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int4 t = tiles[blockIdx.x];  // (list order = tall-window tiles first; an XCD-contiguous order would pile them on one XCD)
  fwd_tile<0, false, 1, 1, EPI>(x, pos, wp, y, d, t.x, t.y, t.z, t.w & 0xffff, smem, epi);
}

// =====================================================================================================================
// Forward on the small-window tiles with the split-bf16 arithmetic of split_arith.h: fp32 operands split exactly
// into three bf16 pieces, six v_mfma_f32_32x32x16_bf16 per product, fp32 accumulation.
//
// Same tile (64 rows x 4 columns), window (81 rows x 8 columns per channel, fp32, double-buffered) and sampling records as
// fwd_tile; what differs is who does what.  K of an MFMA is 16 input channels of one tap, so a chunk is 16 channels deep and
//   * SAMPLING: wave v builds the B fragment of its own 32 pixels (column v % 4, row block v / 4) for tap t + 1 -- 8 channels
//     per lane (lanes 0..31 channels 0..7, lanes 32..63 channels 8..15), 4 LDS words + 4 FMAs each, then the exact 3-way split --
//     and writes the three uint4 to an operand buffer in LDS (2 x 24 KB);
//   * MATRIX: wave v owns output-channel tile v % 4 for the 4 pixel groups of its row block: per tap it reads the 4 x 3
//     fragments the waves of its row block have written and issues 24 MFMAs against ONE weight fragment set (3 KB from L2 per
//     tap and wave -- with all four output tiles per wave, as in fwd_tile, the weights would be 12 KB per tap and wave, and 96 KB per
//     tap for the workgroup through a 64 B/clk L1 lasts as long as the tap's MFMAs at this matrix rate).
// Both run in one instruction stream per wave, the sampling of tap t + 1 under the MFMAs of tap t; one LDS barrier per tap.
// The window of the next chunk is loaded under taps 0..6 and stored under taps 1..7.
// (SP_CCH, SP_CP, SP_WIN, SP_OP and the LDS sizes: sphere_win_internal.h -- the input gradient runs on the same structure)

// F16 of the kernels below: the two-piece fp16 arithmetic (split_arith.h) for the small-window tiles of the TRAINING forward:
// two fp16 pieces per value, three v_mfma_f32_32x32x16_f16 per product (lo x hi, hi x hi, hi x lo).  Both operands are multiplied by
// their tensor's power-of-two scale (f16_scale_of of its largest finite magnitude, a device scalar from the caller); the sampled
// operand gets it through its four bilinear weights, once per tile.  This file splits with split3_bf16_pinned and split2_f16_mix.
// wps[(((((g*MG + mg)*NCH16 + ch)*KT + tap)*MTW + m)*3 + piece)*64 + lane] = 8 bf16: piece of W[g*Cog + mg*128 + m*32 + (lane&31)]
// [ch*16 + 8*(lane>>5) + j][tap], j = 0..7 (scaled by the folded BatchNorm scale when fold != 0; the shifts are the ones pack_w_win wrote)
// F16: two fp16 pieces of w * (the weight tensor's power-of-two scale, from amax_w[0]) in the places of pieces 0 and 1 (no fold)
template <bool F16>
__global__ void pack_w_win_split(const float* __restrict__ w, uint4* __restrict__ wps, WinDims d, int NCH16, int fold, mode_bn_epilogue bn,
                                 const float* __restrict__ amax_w) {
  const float sw = F16 ? f16_scale_of(mode::absmax_load(amax_w)) : 1.f;
  const long long total = (long long)d.G * d.MG * NCH16 * KT * MTW * 64;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    const int lane = (int)(idx & 63);
    long long r = idx >> 6;
    const int m = (int)(r % MTW);
    r /= MTW;
    const int tap = (int)(r % KT);
    r /= KT;
    const int ch = (int)(r % NCH16);
    r /= NCH16;
    const int mg = (int)(r % d.MG);
    const int g = (int)(r / d.MG);
    const int co = mg * 128 + m * 32 + (lane & 31);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = ch * SP_CCH + 8 * (lane >> 5) + j;
      v[j] = 0.f;
      if (co < d.Cog && c < d.Cig) {
        v[j] = w[((long long)(g * d.Cog + co) * d.Cig + c) * KT + tap];
        if (fold) v[j] *= fold_scale(bn, g * d.Cog + co);
        if (F16) v[j] *= sw;
      }
    }
    uint32_t q1[4], q2[4], q3[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if constexpr (F16) {
        split2_f16_mix(v[2 * j], v[2 * j + 1], q1[j], q2[j]);
        q3[j] = 0u;
      } else {
        split3_bf16_pinned(v[2 * j], v[2 * j + 1], q1[j], q2[j], q3[j]);
      }
    }
    uint4* dst = wps + (idx - lane) * 3 + lane;
    dst[0] = make_uint4(q1[0], q1[1], q1[2], q1[3]);
    dst[64] = make_uint4(q2[0], q2[1], q2[2], q2[3]);
    dst[128] = make_uint4(q3[0], q3[1], q3[2], q3[3]);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The TALL-window tiles (next to the poles: windows of 145 rows, or the whole axis with wrap-around) on the same arithmetic (round 4).
// Until then they ran fwd_tile -- fp32 MFMA, matrix-bound, 0.2 ms per tile whatever the image count: the floor of every spherical layer
// of an eval forward at one pair (15 x 0.23 of 11.4 ms) and a third of the training launch.  Their windows do not leave room for an
// operand buffer, so the roles are not split as in the small-tile code below: as in fwd_tile a wave samples its own 32 pixels and
// multiplies them with all four output-channel tiles, straight from registers.  K of one MFMA = 8 input channels x 2 taps (lanes 0..31
// tap 2p, lanes 32..63 tap 2p + 1; five pairs, the second half of the last one multiplies zeros), so a chunk stays 8 channels deep and
// the window staging of fwd_tile is kept as it is.  Per pair and wave: 8 samples per lane (4 LDS words + 4 FMAs each), the exact
// 3-way split, 24 MFMAs against 12 KB of weight fragments (L2 -> L1: what bounds it now: 96 KB per pair and workgroup).
// (TP, the tap pairs of a 3 x 3 kernel: sphere_win_internal.h)

// wpt[(((((g*MG + mg)*NCH + ch)*TP + pair)*MTW + m)*3 + piece)*64 + lane] = 8 bf16: piece of W[g*Cog + mg*128 + m*32 + (lane&31)]
// [ch*8 + j][tap = 2 pair + (lane>>5)], j = 0..7 (zeros for tap 9; scaled by the folded BatchNorm scale when fold != 0)
template <bool F16>
__global__ void pack_w_win_split_tall(const float* __restrict__ w, uint4* __restrict__ wpt, WinDims d, int fold, mode_bn_epilogue bn,
                                      const float* __restrict__ amax_w) {
  const float sw = F16 ? f16_scale_of(mode::absmax_load(amax_w)) : 1.f;
  const long long total = (long long)d.G * d.MG * d.NCH * TP * MTW * 64;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    const int lane = (int)(idx & 63);
    long long r = idx >> 6;
    const int m = (int)(r % MTW);
    r /= MTW;
    const int pair = (int)(r % TP);
    r /= TP;
    const int ch = (int)(r % d.NCH);
    r /= d.NCH;
    const int mg = (int)(r % d.MG);
    const int g = (int)(r / d.MG);
    const int co = mg * 128 + m * 32 + (lane & 31);
    const int tap = 2 * pair + (lane >> 5);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = ch * CCH + j;
      v[j] = 0.f;
      if (tap < KT && co < d.Cog && c < d.Cig) {
        v[j] = w[((long long)(g * d.Cog + co) * d.Cig + c) * KT + tap];
        if (fold) v[j] *= fold_scale(bn, g * d.Cog + co);
        if (F16) v[j] *= sw;
      }
    }
    uint32_t q1[4], q2[4], q3[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if constexpr (F16) {
        split2_f16_mix(v[2 * j], v[2 * j + 1], q1[j], q2[j]);
        q3[j] = 0u;
      } else {
        split3_bf16_pinned(v[2 * j], v[2 * j + 1], q1[j], q2[j], q3[j]);
      }
    }
    uint4* dst = wpt + (idx - lane) * 3 + lane;
    dst[0] = make_uint4(q1[0], q1[1], q1[2], q1[3]);
    dst[64] = make_uint4(q2[0], q2[1], q2[2], q2[3]);
    dst[128] = make_uint4(q3[0], q3[1], q3[2], q3[3]);
  }
}

#ifdef MODE_TAPTIME
__device__ unsigned long long g_taptime[8 * 8192];  // (MODE_STAMP: sphere_win_internal.h)
#endif
// Template parameters as fwd_tile (window rows, double-buffered staging in NPH phases of NRB row passes).
// F16: two fp16 pieces / three MFMAs per product (the small-window code of sphere_fwd_split_kernel<false, true>): a half step is 6 slots.
template <int WR_T, bool PIPE, int NRB, int NPH, bool EPI, bool F16 = false>
__device__ __forceinline__ void fwd_tile_split(const float* __restrict__ x, const float* __restrict__ pos, const uint4* __restrict__ wpt,
                                               float* __restrict__ y, const WinDims& d, int h0, int w0, int rbase, int cbase, float* smem,
                                               const Epi& epi, float sx = 1.f, float unscale = 1.f) {
  const int WRP = WR_T > 0 ? WR_T : d.wr;
  const int CP = chan_pitch(WRP);
  const int bufsz = CCH * CP;
  const int b = blockIdx.y;
  const int g = blockIdx.z / d.MG, mg = blockIdx.z % d.MG;
  MODE_STAMP(0)
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, half = lane >> 5;
  const int h = h0 + (wave / TW) * 32 + (lane & 31), w = w0 + (wave % TW);
  const bool pix_ok = h < d.H && w < d.W;
  const long long HW = (long long)d.H * d.W;

  // sampling records of the taps THIS lane samples: tap 2p + half of pair p (tap 9 does not exist: zero weights)
  int roff[TP];
  float4 rw[TP];
  {
    float ph_[TP], pw_[TP];
    const long long idx = pix_ok ? (long long)h * d.W + w : 0;
#pragma unroll
    for (int p = 0; p < TP; ++p) {
      const int k = min(2 * p + half, KT - 1);
      ph_[p] = pos[(2 * k) * HW + idx];
      pw_[p] = pos[(2 * k + 1) * HW + idx];
    }
#pragma unroll
    for (int p = 0; p < TP; ++p) {
      int r0 = 0, c0 = 0;
      float4 wt = make_float4(0.f, 0.f, 0.f, 0.f);
      mode::tap_record_fixed(ph_[p], pw_[p], d.H, d.W, r0, c0, wt);
      if (!pix_ok || 2 * p + half >= KT) wt = make_float4(0.f, 0.f, 0.f, 0.f);
      int lr = r0 - rbase;
      if (lr < 0) lr += d.H;
      const int lc = c0 - cbase;
      const bool dead = wt.x == 0.f && wt.y == 0.f && wt.z == 0.f && wt.w == 0.f;
      roff[p] = dead ? 0 : lc * WRP + lr;
      rw[p] = F16 ? make_float4(wt.x * sx, wt.y * sx, wt.z * sx, wt.w * sx) : wt;  // (the operand's power-of-two scale rides on the weights)
    }
  }
  const int lds_floats = (PIPE ? 2 : 1) * bufsz + WRP + 8;
  for (int i = tid; i < lds_floats; i += NTHREADS) smem[i] = 0.f;  // every window word that may be read is finite
  __syncthreads();

  // window staging: exactly fwd_tile's
  const int scol = d.sh == 1 ? tid / SROWS : tid & (WC - 1), srow = d.sh == 1 ? tid % SROWS : tid / WC;
  const int gcol = cbase + scol;
  const bool col_ok = gcol < d.W;
  const float* xg = x + ((long long)b * d.Ci + (long long)g * d.Cig) * HW + (col_ok ? gcol * d.sw : 0);
  int rowoff[NRB];
#pragma unroll
  for (int rb = 0; rb < NRB; ++rb) {
    const int r = rb * SROWS + srow;
    rowoff[rb] = ((rbase + (r < WRP ? r : 0)) % d.H) * d.sh;
  }
  constexpr int CPH = CCH / NPH;
  float lv[PIPE ? CPH * NRB : 1];
  auto issue = [&](int ch, int ph) {
#pragma unroll
    for (int cc = 0; cc < CPH; ++cc) {
      const int chan = ch * CCH + ph * CPH + cc;
      const float* xc = xg + (long long)(chan < d.Cig ? chan : 0) * HW;
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb) lv[cc * NRB + rb] = xc[rowoff[rb]];
    }
  };
  auto commit = [&](int ch, int ph, float* buf) {
#pragma unroll
    for (int cc = 0; cc < CPH; ++cc) {
      const int c = ph * CPH + cc;
      const bool ok = col_ok && (ch * CCH + c < d.Cig);
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb) {
        const int r = rb * SROWS + srow;
        if (r < WRP) buf[c * CP + scol * WRP + r] = ok ? lv[cc * NRB + rb] : 0.f;
      }
    }
  };
  f32x16 acc[MTW];
#pragma unroll
  for (int m = 0; m < MTW; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;

  // WEIGHT FRAGMENTS THROUGH LDS (round 4).  A pair step multiplies this wave's B fragment with all four output tiles: 12 fragments =
  // 12 KB, the same for the 8 waves.  Fetched by every wave on its own they were 96 KB per step and workgroup through the vector
  // memory path (L1 holds 32 KB; a chunk's five steps are 60 KB), and a tall tile took 0.18 ms against 0.09 ms for a small-window
  // tile -- the critical path of the launch at 2 and 4 images.  Now the workgroup fetches a step's 12 KB once (1.5 x 16 B per thread),
  // one step ahead, into one of two LDS buffers behind the windows, and the waves read their fragments from there.  One barrier per
  // step, in its middle: first half = tiles 0, 1 (fragments read during the second half of the previous step), second half = tiles
  // 2, 3 (read during the first half); the next step's weights are stored at the top of a step and visible after its barrier.
  // The sampling arithmetic of the next step sits between the MFMAs slot by slot (see sphere_fwd_split_kernel).
  static_assert(PIPE, "the split tall tiles are double-buffered");
  constexpr int WSTEP = MTW * 3 * 64;  // uint4 per pair step
  uint4* wbuf = reinterpret_cast<uint4*>(smem + ((lds_floats + 3) / 4) * 4);  // [2][WSTEP]
  const uint4* wsrc = wpt + ((long long)(g * d.MG + mg) * d.NCH) * TP * WSTEP;  // + step * WSTEP + fragment * 64 + lane
  const int nsteps = d.NCH * TP;
  uint4 wg0, wg1;  // the 1.5 x 16 bytes this thread fetches of the step after the next
  auto wfetch = [&](int step) {
    const uint4* src = wsrc + (long long)(step < nsteps ? step : nsteps - 1) * WSTEP;
    wg0 = src[tid];
    wg1 = src[NTHREADS + (tid & 255)];
  };
  auto wstore = [&](int step) {
    uint4* dst = wbuf + (step & 1) * WSTEP;
    dst[tid] = wg0;
    if (tid < 256) dst[NTHREADS + tid] = wg1;
  };
  wfetch(0);

  // the 8 channel values of this lane's (pixel, tap) for pair p: 32 window words, then 4 FMAs each and the split
  float raw[16], v[8], ra[4], rb[4];  // window words of HALF a sample set (4 channels), requested in two batches per step
  uint32_t q1[4], q2[4], q3[4];
  auto load_half = [&](const float* buf, int p, int hb) {
    const float* q0 = buf + roff[p] + hb * 4 * CP;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float* q = q0 + c * CP;
      raw[c * 4 + 0] = q[0];
      raw[c * 4 + 1] = q[WRP];
      raw[c * 4 + 2] = q[1];
      raw[c * 4 + 3] = q[WRP + 1];
    }
  };
  auto comb = [&](int p, int c) {  // (one scalar chain per value: see sphere_fwd_split_kernel)
    const float4 tw = rw[p];
    const int r = (c & 3) * 4;
    v[c] = __builtin_fmaf(tw.w, raw[r + 3], __builtin_fmaf(tw.z, raw[r + 2], __builtin_fmaf(tw.y, raw[r + 1], tw.x * raw[r])));
    asm("" : "+v"(v[c]));
  };
  auto split_a = [&](int j) {
    ra[j] = v[2 * j];
    rb[j] = v[2 * j + 1];
    q1[j] = split_step_bf16_pinned(ra[j], rb[j]);
  };
  auto split_b = [&](int j) { q2[j] = split_step_bf16_pinned(ra[j], rb[j]); };
  auto split_c = [&](int j) { q3[j] = pack2(ra[j], rb[j]); };
  auto hsplit = [&](int j) { split2_f16_mix(v[2 * j], v[2 * j + 1], q1[j], q2[j]); };

#pragma unroll
  for (int ph = 0; ph < NPH; ++ph) {
    issue(0, ph);
    commit(0, ph, smem);
  }
  wstore(0);
  wfetch(1);
  __syncthreads();
  uint4 a_cur[2][3], a_nxt[2][3], bq[3];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int q = 0; q < 3; ++q) a_cur[m][q] = wbuf[(m * 3 + q) * 64 + lane];
  constexpr int PPP = TP / NPH;  // tap pairs per staging phase (NPH = 2: pairs 0-1 | 2-4; NPH = 4: one pair each, the last phase two)
  // B fragment of the first pair of the first chunk; every later one is built under the MFMAs of the step before it -- the first pair
  // of a chunk too: the last phase of the next chunk's window is stored in the FIRST half of the chunk's last step, so that window is
  // complete at that step's barrier and its second half can sample from it (no chunk-top sampling, no barrier at the chunk end)
  load_half(smem, 0, 0);
#pragma unroll
  for (int c = 0; c < 4; ++c) comb(0, c);
  load_half(smem, 0, 1);
#pragma unroll
  for (int c = 4; c < 8; ++c) comb(0, c);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if constexpr (F16) {
      hsplit(j);
      q3[j] = 0u;
    } else {
      split_a(j);
      split_b(j);
      split_c(j);
    }
  }
  bq[0] = make_uint4(q1[0], q1[1], q1[2], q1[3]);
  bq[1] = make_uint4(q2[0], q2[1], q2[2], q2[3]);
  bq[2] = make_uint4(q3[0], q3[1], q3[2], q3[3]);
  load_half(smem, 1, 0);  // first half batch of the fragment built under step 0
  MODE_STAMP(1)
#ifdef MODE_TAPTIME
  unsigned long long tt_top = 0, tt_pre = 0, tt_post = __builtin_readcyclecounter(), ts_a = 0, ts_b = 0, ts_c = 0;
#endif
  for (int ch = 0; ch < d.NCH; ++ch) {
    float* cur = smem + (ch & 1) * bufsz;
    float* nxt = smem + ((ch + 1) & 1) * bufsz;
    const bool more = ch + 1 < d.NCH;
#pragma unroll
    for (int p = 0; p < TP; ++p) {
      const int step = ch * TP + p;
      const uint4* wcur = wbuf + (step & 1) * WSTEP + lane;
      const uint4* wnx = wbuf + ((step + 1) & 1) * WSTEP + lane;
      const int pn = p + 1 < TP ? p + 1 : 0;  // the pair whose B fragment is built under this step (pair 0 of the next chunk under the last)
      // ---- first half: output tiles 0, 1.  LDS traffic is spread over the slots (requested in one batch at the top, the 24 reads and
      // stores of the 8 waves backed up in front of the first MFMA: 1 650 cycles for this half against 930 for the other)
#ifdef MODE_TAPTIME
      tt_top = __builtin_readcyclecounter();
#endif
      if constexpr (F16) {
        // 6 slots: lo x hi, hi x lo, hi x hi for tiles 0 and 1; the rest of the step's LDS and sampling work between them as below
        MODE_SB
        MODE_TMFH(1, 0, 0, 0) if (p + 1 < TP) comb(pn, 0); MODE_SB
        MODE_TMFH(1, 0, 1, 1) if (p + 1 < TP) comb(pn, 1); MODE_SB
        MODE_TMFH(0, 1, 0, 0) if (p + 1 < TP) comb(pn, 2); wstore(step + 1); MODE_SB
        MODE_TMFH(0, 1, 1, 1) if (p + 1 < TP) comb(pn, 3); wfetch(step + 2); MODE_SB
        if (p + 1 < TP) load_half(cur, pn, 1);
        if (p % PPP == 0 && p / PPP < NPH && more) issue(ch + 1, p / PPP);
        if (p == TP - 1 && more) commit(ch + 1, NPH - 1, nxt);
#pragma unroll
        for (int q = 0; q < 2; ++q) a_nxt[0][q] = wcur[((2 + 0) * 3 + q) * 64];
#pragma unroll
        for (int q = 0; q < 2; ++q) a_nxt[1][q] = wcur[((2 + 1) * 3 + q) * 64];
        MODE_SB
        MODE_TMFH(0, 0, 0, 0) if (p + 1 < TP) { comb(pn, 4); comb(pn, 5); } MODE_SB
        MODE_TMFH(0, 0, 1, 1) if (p + 1 < TP) { comb(pn, 6); comb(pn, 7); } MODE_SB
      } else {
      MODE_SB
      MODE_TMF(2, 0, 0, 0) if (p + 1 < TP) comb(pn, 0); MODE_SB
      MODE_TMF(2, 0, 1, 1) if (p + 1 < TP) comb(pn, 1); MODE_SB
      MODE_TMF(0, 2, 0, 0) if (p + 1 < TP) comb(pn, 2); wstore(step + 1); MODE_SB
      MODE_TMF(0, 2, 1, 1) if (p + 1 < TP) comb(pn, 3); wfetch(step + 2); MODE_SB
      if (p + 1 < TP) load_half(cur, pn, 1);
      if (p % PPP == 0 && p / PPP < NPH && more) issue(ch + 1, p / PPP);  // rows of the next chunk fly under the MFMAs below
      if (p == TP - 1 && more) commit(ch + 1, NPH - 1, nxt);  // (its loads were requested a step ago)
      MODE_SB
      MODE_TMF(1, 1, 0, 0) MODE_SB
#pragma unroll
      for (int q = 0; q < 3; ++q) a_nxt[0][q] = wcur[((2 + 0) * 3 + q) * 64];
      MODE_SB
      MODE_TMF(1, 1, 1, 1) MODE_SB
#pragma unroll
      for (int q = 0; q < 3; ++q) a_nxt[1][q] = wcur[((2 + 1) * 3 + q) * 64];
      MODE_SB
      MODE_TMF(1, 0, 0, 0) if (p + 1 < TP) comb(pn, 4); MODE_SB
      MODE_TMF(1, 0, 1, 1) if (p + 1 < TP) comb(pn, 5); MODE_SB
      MODE_TMF(0, 1, 0, 0) if (p + 1 < TP) comb(pn, 6); MODE_SB
      MODE_TMF(0, 1, 1, 1) if (p + 1 < TP) comb(pn, 7); MODE_SB
      MODE_TMF(0, 0, 0, 0) MODE_SB
      MODE_TMF(0, 0, 1, 1) MODE_SB
      }
#ifdef MODE_TAPTIME
      tt_pre = __builtin_readcyclecounter();
#endif
      lds_barrier();  // the weights of step + 1 are in LDS
#ifdef MODE_TAPTIME
      ts_c += tt_top - tt_post;  // second half of the previous step
      tt_post = __builtin_readcyclecounter();
      ts_a += tt_pre - tt_top;
      ts_b += tt_post - tt_pre;
#endif
      // ---- second half: output tiles 2, 3
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int q = 0; q < 3; ++q) a_cur[m][q] = a_nxt[m][q];
      if (p + 1 == TP) load_half(more ? nxt : cur, 0, 0);  // (after the last chunk: any finite words, the fragment is not used)
      MODE_SB
      if constexpr (F16) {
        if (p + 1 < TP) {
          MODE_TMFH(1, 0, 0, 2) hsplit(0); MODE_SB
          MODE_TMFH(1, 0, 1, 3) hsplit(1); MODE_SB
#pragma unroll
          for (int q = 0; q < 2; ++q) a_nxt[0][q] = wnx[(0 * 3 + q) * 64];
          MODE_SB
          MODE_TMFH(0, 1, 0, 2) hsplit(2); MODE_SB
          MODE_TMFH(0, 1, 1, 3) hsplit(3); MODE_SB
#pragma unroll
          for (int q = 0; q < 2; ++q) a_nxt[1][q] = wnx[(1 * 3 + q) * 64];
          if (p + 2 < TP) load_half(cur, p + 2, 0);  // first half batch of the fragment built under the next step
          MODE_SB
          MODE_TMFH(0, 0, 0, 2) MODE_SB
          MODE_TMFH(0, 0, 1, 3) MODE_SB
        } else {  // the whole B fragment of the next chunk's first pair under these six MFMAs
          MODE_TMFH(1, 0, 0, 2) comb(0, 0); comb(0, 1); MODE_SB
          MODE_TMFH(1, 0, 1, 3) comb(0, 2); comb(0, 3); MODE_SB
          load_half(more ? nxt : cur, 0, 1);
#pragma unroll
          for (int q = 0; q < 2; ++q) a_nxt[0][q] = wnx[(0 * 3 + q) * 64];
#pragma unroll
          for (int q = 0; q < 2; ++q) a_nxt[1][q] = wnx[(1 * 3 + q) * 64];
          MODE_SB
          MODE_TMFH(0, 1, 0, 2) MODE_SB
          MODE_TMFH(0, 1, 1, 3) comb(0, 4); comb(0, 5); comb(0, 6); comb(0, 7); MODE_SB
          load_half(more ? nxt : cur, 1, 0);  // (the fragment built under the next chunk's first step)
          MODE_SB
          MODE_TMFH(0, 0, 0, 2) hsplit(0); hsplit(1); MODE_SB
          MODE_TMFH(0, 0, 1, 3) hsplit(2); hsplit(3); MODE_SB
        }
      } else
      if (p + 1 < TP) {
        MODE_TMF(2, 0, 0, 2) split_a(0); MODE_SB
        MODE_TMF(2, 0, 1, 3) split_b(0); MODE_SB
#pragma unroll
        for (int q = 0; q < 3; ++q) a_nxt[0][q] = wnx[(0 * 3 + q) * 64];
        MODE_SB
        MODE_TMF(0, 2, 0, 2) split_c(0); split_a(1); MODE_SB
        MODE_TMF(0, 2, 1, 3) split_b(1); MODE_SB
#pragma unroll
        for (int q = 0; q < 3; ++q) a_nxt[1][q] = wnx[(1 * 3 + q) * 64];
        MODE_SB
        MODE_TMF(1, 1, 0, 2) split_c(1); split_a(2); MODE_SB
        MODE_TMF(1, 1, 1, 3) split_b(2); MODE_SB
        MODE_TMF(1, 0, 0, 2) split_c(2); split_a(3); MODE_SB
        MODE_TMF(1, 0, 1, 3) split_b(3); MODE_SB
        MODE_TMF(0, 1, 0, 2) split_c(3); MODE_SB
        if (p + 2 < TP) load_half(cur, p + 2, 0);  // first half batch of the fragment built under the next step
        MODE_SB
        MODE_TMF(0, 1, 1, 3) MODE_SB
        MODE_TMF(0, 0, 0, 2) MODE_SB
        MODE_TMF(0, 0, 1, 3) MODE_SB
      } else {  // the whole B fragment of the next chunk's first pair under these twelve MFMAs
        MODE_TMF(2, 0, 0, 2) MODE_SB
        MODE_TMF(2, 0, 1, 3) MODE_SB
        MODE_TMF(0, 2, 0, 2) comb(0, 0); comb(0, 1); MODE_SB
        MODE_TMF(0, 2, 1, 3) comb(0, 2); comb(0, 3); MODE_SB
        load_half(more ? nxt : cur, 0, 1);
#pragma unroll
        for (int q = 0; q < 3; ++q) a_nxt[0][q] = wnx[(0 * 3 + q) * 64];
        MODE_SB
        MODE_TMF(1, 1, 0, 2) MODE_SB
#pragma unroll
        for (int q = 0; q < 3; ++q) a_nxt[1][q] = wnx[(1 * 3 + q) * 64];
        MODE_SB
        MODE_TMF(1, 1, 1, 3) MODE_SB
        MODE_TMF(1, 0, 0, 2) comb(0, 4); comb(0, 5); MODE_SB
        MODE_TMF(1, 0, 1, 3) comb(0, 6); comb(0, 7); MODE_SB
        load_half(more ? nxt : cur, 1, 0);  // (the fragment built under the next chunk's first step)
        MODE_SB
        MODE_TMF(0, 1, 0, 2) split_a(0); split_a(1); split_a(2); MODE_SB
        MODE_TMF(0, 1, 1, 3) split_a(3); split_b(0); split_b(1); MODE_SB
        MODE_TMF(0, 0, 0, 2) split_b(2); split_b(3); split_c(0); MODE_SB
        MODE_TMF(0, 0, 1, 3) split_c(1); split_c(2); split_c(3); MODE_SB
      }
      if (more && p < TP - 1 && p % PPP == PPP - 1 && p / PPP < NPH - 1) commit(ch + 1, p / PPP, nxt);  // the other buffer: nobody reads it now
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int q = 0; q < 3; ++q) a_cur[m][q] = a_nxt[m][q];
      bq[0] = make_uint4(q1[0], q1[1], q1[2], q1[3]);
      bq[1] = make_uint4(q2[0], q2[1], q2[2], q2[3]);
      bq[2] = make_uint4(q3[0], q3[1], q3[2], q3[3]);
    }
  }
  MODE_STAMP(2)
#ifdef MODE_TAPTIME
  MODE_STAMPV(4, ts_a)
  MODE_STAMPV(5, ts_b)
  MODE_STAMPV(6, ts_c)
#endif

  if (pix_ok) {
    float* yb = y + ((long long)b * d.Co + (long long)g * d.Cog + (long long)mg * 128) * HW + (long long)h * d.sh + (long long)w * d.sw;
    const int cmax = d.Cog - mg * 128;
#pragma unroll
    for (int m = 0; m < MTW; ++m) {
      // (eval mode: the 16 shifts and the 16 residual values of this M-tile are requested TOGETHER ahead of its stores, under one uniform
      // test each: read inside the store loop every store waited for a load of its own -- see sphere_fwd_split_kernel's epilogue)
      float res[16], shv[16];
      if (EPI) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int co = min(MODE_ACC_ROW(m, r, half), cmax - 1);
          shv[r] = epi.shift[g * d.Cog + mg * 128 + co];
          res[r] = 0.f;
        }
        if (epi.add) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int co = min(MODE_ACC_ROW(m, r, half), cmax - 1);
            res[r] = epi.add[(yb - y) + (long long)co * HW];
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      auto emit = [&](int r) {
        const int co = MODE_ACC_ROW(m, r, half);
        if (EPI) {
          const float v = (acc[m][r] + shv[r]) + res[r];
          yb[(long long)co * HW] = epi.relu ? relu_nan(v) : v;
        } else {
          yb[(long long)co * HW] = F16 ? acc[m][r] * unscale : acc[m][r];
        }
      };
      if (m * 32 + 32 <= cmax) {  // (uniform) a full M-tile: no test per store
#pragma unroll
        for (int r = 0; r < 16; ++r) emit(r);
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (MODE_ACC_ROW(m, r, half) < cmax) emit(r);
      }
      if (EPI) __builtin_amdgcn_sched_barrier(0);
    }
  }
  MODE_STAMP(3)
}

// F16 (training forward, no epilogue): two fp16 pieces and three MFMAs per product -- a tap of the small-window tiles is 12 slots
// instead of 24, and the split of a sampled value 3 instructions instead of 5.5; the tall-window tiles (fwd_tile_split<.., F16>) likewise.
template <bool EPI, bool F16 = false>
__global__ __launch_bounds__(NTHREADS) void sphere_fwd_split_kernel(const float* __restrict__ x, const float* __restrict__ pos,
                                                                    const uint4* __restrict__ wps, const uint4* __restrict__ wpt,
                                                                    float* __restrict__ y, WinDims d, int NCH16,
                                                                    const int4* __restrict__ tiles, Epi epi,
                                                                    const float* __restrict__ amax_x, const float* __restrict__ amax_w) {
  static_assert(!(EPI && F16), "the fp16 arithmetic has no folded-BatchNorm epilogue");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int WRP = WR_SMALL, CP = SP_CP;
  uint4* opbuf = reinterpret_cast<uint4*>(smem + SP_WIN_FLOATS);  // [3][8 pixel groups][3 pieces][64 lanes]
  const int4 t = tiles[blockIdx.x];
  const int h0 = t.x, w0 = t.y, rbase = t.z, cbase = t.w & 0xffff;
  // the few tall-window tiles (next to the poles) run INSIDE this launch (as a launch of their own they would be an under-filled tail:
  // 0.37 ms for the two launches against 0.26 for the old single one), on the same arithmetic since round 4 (fwd_tile_split)
  const int cls = t.w >> 16;
  if (cls == 1) {
    if constexpr (F16) {
      const float sx_ = f16_scale_of(mode::absmax_load(amax_x));
      fwd_tile_split<WR_MID, true, (WR_MID + SROWS - 1) / SROWS, 2, EPI, true>(x, pos, wpt, y, d, t.x, t.y, t.z, cbase, smem, epi, sx_,
                                                                              (1.f / sx_) * (1.f / f16_scale_of(mode::absmax_load(amax_w))));
    } else {
      fwd_tile_split<WR_MID, true, (WR_MID + SROWS - 1) / SROWS, 2, EPI>(x, pos, wpt, y, d, t.x, t.y, t.z, cbase, smem, epi);
    }
    return;
  }
  if (cls != 0) {
    if constexpr (F16) {
      const float sx_ = f16_scale_of(mode::absmax_load(amax_x));
      fwd_tile_split<0, true, WR_PIPE_MAX / SROWS, 4, EPI, true>(x, pos, wpt, y, d, t.x, t.y, t.z, cbase, smem, epi, sx_,
                                                                 (1.f / sx_) * (1.f / f16_scale_of(mode::absmax_load(amax_w))));
    } else {
      fwd_tile_split<0, true, WR_PIPE_MAX / SROWS, 4, EPI>(x, pos, wpt, y, d, t.x, t.y, t.z, cbase, smem, epi);
    }
    return;
  }
  MODE_STAMP(0)
  const int b = blockIdx.y;
  const int g = blockIdx.z / d.MG, mg = blockIdx.z % d.MG;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, half = lane >> 5;
  const int h = h0 + (wave / TW) * 32 + (lane & 31), w = w0 + (wave % TW);  // the pixel this lane SAMPLES
  const bool pix_ok = h < d.H && w < d.W;
  const long long HW = (long long)d.H * d.W;
  float sx = 1.f, unscale = 1.f;
  if (F16) {
    sx = f16_scale_of(mode::absmax_load(amax_x));
    unscale = (1.f / sx) * (1.f / f16_scale_of(mode::absmax_load(amax_w)));
  }

  int roff[KT];
  float4 rw[KT];
  // (all 18 table values first, from a clamped index: inside `if (pix_ok)` they were nine dependent load -> compute rounds, and the
  // prologue of a tile is not overlapped with anything)
  float ph_[KT], pw_[KT];
  {
    const long long idx = pix_ok ? (long long)h * d.W + w : 0;
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      ph_[k] = pos[(2 * k) * HW + idx];
      pw_[k] = pos[(2 * k + 1) * HW + idx];
    }
  }
  // every window word that may be read is finite: the staging stores write all rows and columns of both windows; what they never
  // write is the pad word behind each channel and the slack behind the two buffers (read only under zero weights)
  if (tid < 2 * SP_CCH) smem[(tid / SP_CCH) * SP_WIN + (tid % SP_CCH) * CP + WC * WRP] = 0.f;
  if (tid < WRP + 8) smem[SP_WIN + tid] = 0.f;  // (the last channel of the first window runs over into the second, which is empty during the first chunk)
  for (int i = 2 * SP_WIN + tid; i < SP_WIN_FLOATS; i += NTHREADS) smem[i] = 0.f;
  // (no barrier here: it would drain the table loads above before the first window is even requested -- 9 k of a workgroup's 190 k
  // cycles.  The only words both this fill and the staging stores below write are slack words, where either value will do; the barrier
  // behind the staging stores orders everything in front of the first sample)
  MODE_STAMP(4)

  // window staging: thread -> (window column, row within a pass of SROWS rows), as in fwd_tile; 2 passes cover the 81 rows
  const int scol = d.sh == 1 ? tid / SROWS : tid & (WC - 1), srow = d.sh == 1 ? tid % SROWS : tid / WC;
  const int gcol = cbase + scol;
  const bool col_ok = gcol < d.W;
  const float* xg = x + ((long long)b * d.Ci + (long long)g * d.Cig) * HW;  // uniform; lanes add 32-bit element offsets (H * W < 2^30)
  unsigned rowoff[2];  // BYTE offsets inside a channel plane
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    const int r = rb * SROWS + srow;
    rowoff[rb] = 4u * (unsigned)(((rbase + (r < WRP ? r : 0)) % d.H) * d.sh + (col_ok ? gcol * d.sw : 0));
  }
  const long long plane_bytes = 4 * HW;
  constexpr int STAGE_LAG = 2;  // taps between the loads of a staging phase and its LDS stores
  float lv[8][4];  // the 8 staging phases of a chunk (phase = 2 channels x 2 row passes), all in flight at once
  auto issue = [&](int ch, int ph, int set) {  // (Cig is a multiple of 16: every channel of a chunk exists)
    const char* xc = reinterpret_cast<const char*>(xg) + ((long long)ch * SP_CCH + ph * 2) * plane_bytes;  // uniform
#pragma unroll
    for (int cc = 0; cc < 2; ++cc)
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) lv[set][cc * 2 + rb] = *reinterpret_cast<const float*>(xc + cc * plane_bytes + rowoff[rb]);
  };
  auto commit = [&](int ch, int ph, int set, float* buf) {
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
      const int c = ph * 2 + cc;
      const bool ok = col_ok;
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) {
        // rows beyond the window go to the slack words behind the two buffers (finite values, read only under zero weights): an
        // `if` here is a branch, and a branch in the middle of a tap pins the sampling code behind the MFMAs
        const int r = rb * SROWS + srow;
        float* dst = r < WRP ? buf + c * CP + scol * WRP + r : smem + 2 * SP_WIN + (tid & 7);
        *dst = ok ? lv[set][cc * 2 + rb] : 0.f;
      }
    }
  };
  // B fragment of this lane's pixel for tap k of the chunk in `win`: 8 channels, split, stored as this wave's group.  In two halves:
  // sample_read requests the 32 window words (16 ds_read2_b32) in ONE batch, sample_finish combines, splits and stores them.  As one
  // lambda the compiler issued each read right in front of its use (`ds_read2_b32; s_waitcnt lgkmcnt(0)` sixteen times per tap, all
  // of it BEHIND the tap's 24 MFMAs): sixteen serialised LDS round trips per tap and wave, 2 700 cycles per tap against the 1 536 the
  // matrix pipe needs (tools/experiments/tap_pipeline.hip reproduces it without the rest of the kernel)
  auto sample_read = [&](const float* win, int k, float (&raw)[8][4]) {
    const float* p = win + half * 8 * CP + roff[k];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float* q = p + c * CP;
      raw[c][0] = q[0];
      raw[c][1] = q[WRP];
      raw[c][2] = q[1];
      raw[c][3] = q[WRP + 1];
    }
  };
  auto sample_finish = [&](int k, float (&raw)[8][4], uint4* op) {
    const float4 tw = rw[k];
    float v[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      // (one fma chain per value: left to itself the compiler SLP-packs these into v_pk_fma_f32, which costs the MFMA stream more
      // than two plain FMAs)
      v[c] = __builtin_fmaf(tw.w, raw[c][3], __builtin_fmaf(tw.z, raw[c][2], __builtin_fmaf(tw.y, raw[c][1], tw.x * raw[c][0])));
      asm("" : "+v"(v[c]));  // (opaque, not volatile -- a volatile asm pins the schedule: keeps the chains of two channels from being packed pairwise -- 24 v_mov + 24 v_pk_*)
    }
    uint32_t q1[4], q2[4], q3[4];
    uint4* dst = op + (wave * 3) * 64 + lane;
    if constexpr (F16) {
#pragma unroll
      for (int j = 0; j < 4; ++j) split2_f16_mix(v[2 * j], v[2 * j + 1], q1[j], q2[j]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) split3_bf16_pinned(v[2 * j], v[2 * j + 1], q1[j], q2[j], q3[j]);
      dst[128] = make_uint4(q3[0], q3[1], q3[2], q3[3]);
    }
    dst[0] = make_uint4(q1[0], q1[1], q1[2], q1[3]);
    dst[64] = make_uint4(q2[0], q2[1], q2[2], q2[3]);
  };
  auto sample = [&](const float* win, int k, uint4* op) {
    float raw[8][4];
    sample_read(win, k, raw);
    __builtin_amdgcn_sched_barrier(0);  // (all 16 reads requested before the first one is used)
    sample_finish(k, raw, op);
  };

  f32x16 acc[4];
#pragma unroll
  for (int gi = 0; gi < 4; ++gi)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[gi][r] = 0.f;
  const int m = wave % TW, gset = (wave / TW) * 4;  // output tile and first pixel group of the MATRIX role
  const uint4* wpa = wps + ((long long)(g * d.MG + mg) * NCH16) * KT * MTW * 192 + m * 192;  // uniform; + p * 64 + lane per fragment
  const int nsteps = NCH16 * KT;
  constexpr int NPC = Arith<F16>::NP;  // pieces per value
  uint4 acur[3], anxt[3];  // weight fragments of this tap and of the next one (requested at the top of a tap, one tap ahead)
#pragma unroll
  for (int p = 0; p < NPC; ++p) acur[p] = wpa[(unsigned)(p * 64 + lane)];

  // prologue: window of chunk 0, operand of tap 0
#pragma unroll
  for (int ph = 0; ph < 8; ++ph) issue(0, ph, ph);  // 32 loads in flight, then the stores: one memory round trip, not eight
  // (the sampling records are computed while those loads fly)
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    int r0 = 0, c0 = 0;
    float4 wt = make_float4(0.f, 0.f, 0.f, 0.f);
    mode::tap_record_fixed(ph_[k], pw_[k], d.H, d.W, r0, c0, wt);
    if (!pix_ok) wt = make_float4(0.f, 0.f, 0.f, 0.f);
    int lr = r0 - rbase;
    if (lr < 0) lr += d.H;
    const int lc = c0 - cbase;
    const bool dead = wt.x == 0.f && wt.y == 0.f && wt.z == 0.f && wt.w == 0.f;
    roff[k] = (dead || !pix_ok) ? 0 : lc * WRP + lr;
    // (F16: the operand's power-of-two scale rides on the four weights -- sx * (sum of w_i x_i) bit for bit, no instruction per sample)
    rw[k] = F16 ? make_float4(wt.x * sx, wt.y * sx, wt.z * sx, wt.w * sx) : wt;
  }
  MODE_STAMP(5)
#pragma unroll
  for (int ph = 0; ph < 8; ++ph) commit(0, ph, ph, smem);
  __syncthreads();
  MODE_STAMP(6)
  // ---- the tap loop.  Three operand buffers: tap t multiplies fragments of buffer t % 3, samples tap t + 2 into buffer (t + 2) % 3 and
  // reads piece 0 of tap t + 1 near its end, so no MFMA waits for an LDS read of its own tap.  A tap is 24 SLOTS (one MFMA each) with
  // everything else placed by hand between them and fenced with sched_barrier(0): left to the scheduler, the window reads ended up
  // one by one in front of their uses, behind all 24 MFMAs (see sample_read above).  Fragment registers: piece 0 (slots 0..11), piece
  // 1 (read in slot 4, used 12..19), piece 2 (read in slot 12, used 20..23), piece 0 of the next tap (read in slot 20) -- never more
  // than two of the four sets alive.  Window words: two half batches of 4 channels (16 registers), the second requested in slot 4
  // when the first has been consumed.  Measured on the skeleton of this loop (tools/experiments/tap_pipeline.hip, gen_tap_asm.py):
  // 2 750 cycles per tap as it was, ~2 100 in this form, 1 500 for the MFMAs alone.
  sample(smem, 0, opbuf);
  sample(smem, 1, opbuf + SP_OP);
  lds_barrier();
  uint4 b0[4], b0n[4], b1[4], b2[4];
  const uint4* fragbase = opbuf + gset * 192 + lane;  // + buffer * SP_OP + (gi * 3 + piece) * 64
#pragma unroll
  for (int gi = 0; gi < 4; ++gi) b0[gi] = fragbase[(gi * 3 + 0) * 64];
  float raw[4][4], v[8], ra[4], rb[4];
  uint32_t q1[4], q2[4], q3[4];
  {
    const float* wp0 = smem + half * 8 * CP + roff[2];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float* q = wp0 + c * CP;
      raw[c][0] = q[0];
      raw[c][1] = q[WRP];
      raw[c][2] = q[1];
      raw[c][3] = q[WRP + 1];
    }
  }
  MODE_STAMP(1)
  if constexpr (F16) {
    // ---- 12 slots: lo x hi (piece 1 of the weights against piece 0 of the operand), hi x hi, hi x lo.  The second half batch of window
    // words has registers of its own (the third piece's are free) and is requested at the top of the tap; the next tap's first half batch
    // and its piece-0 fragments in slot 8, when the combines have consumed this tap's.
    float raw2[4][4];
    for (int ch = 0; ch < NCH16; ++ch) {
      float* cur = smem + (ch & 1) * SP_WIN;
      float* nxt = smem + ((ch + 1) & 1) * SP_WIN;
      const int chn = ch + 1 < NCH16 ? ch + 1 : ch;
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        const int step = ch * KT + k;
        const int nstep = step + 1 < nsteps ? step + 1 : nsteps - 1;
        const int ks = (k + 2) % KT;
        const float* wsrc = k + 2 < KT ? cur : nxt;
        const uint4* fcur = fragbase + (k % 3) * SP_OP;
        const uint4* fnxt = fragbase + ((k + 1) % 3) * SP_OP;
        uint4* opw = opbuf + ((k + 2) % 3) * SP_OP + (wave * 3) * 64 + lane;
        const float4 tw = rw[ks];
        const float* wp_ = wsrc + half * 8 * CP + roff[ks];
        const float* wpn_ = (k + 3 < KT ? cur : nxt) + half * 8 * CP + roff[(k + 3) % KT];
        auto combine = [&](int c, float (&rr)[4][4]) {  // (one fma chain per value, kept scalar: see split3_bf16_pinned)
          v[c] = __builtin_fmaf(tw.w, rr[c & 3][3], __builtin_fmaf(tw.z, rr[c & 3][2], __builtin_fmaf(tw.y, rr[c & 3][1], tw.x * rr[c & 3][0])));
          asm("" : "+v"(v[c]));
        };
        auto hsplit = [&](int j) { split2_f16_mix(v[2 * j], v[2 * j + 1], q1[j], q2[j]); };
#pragma unroll
        for (int p = 0; p < 2; ++p) anxt[p] = (wpa + (long long)nstep * MTW * 192)[(unsigned)(p * 64 + lane)];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float* q = wp_ + (4 + c) * CP;
          raw2[c][0] = q[0];
          raw2[c][1] = q[WRP];
          raw2[c][2] = q[1];
          raw2[c][3] = q[WRP + 1];
        }
#pragma unroll
        for (int gi = 0; gi < 4; ++gi) b1[gi] = fcur[(gi * 3 + 1) * 64];
        MODE_SB
        MODE_MFH(0, b0, 0) combine(0, raw); MODE_SB
        MODE_MFH(0, b0, 1) combine(1, raw); MODE_SB
        MODE_MFH(0, b0, 2) combine(2, raw); MODE_SB
        MODE_MFH(0, b0, 3) combine(3, raw); MODE_SB
        MODE_MFH(1, b0, 0) hsplit(0); MODE_SB
        MODE_MFH(1, b0, 1) hsplit(1); combine(4, raw2); MODE_SB
        MODE_MFH(1, b0, 2) combine(5, raw2); combine(6, raw2); MODE_SB
        MODE_MFH(1, b0, 3) combine(7, raw2); MODE_SB
#pragma unroll
        for (int gi = 0; gi < 4; ++gi) b0n[gi] = fnxt[(gi * 3 + 0) * 64];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float* q = wpn_ + c * CP;
          raw[c][0] = q[0];
          raw[c][1] = q[WRP];
          raw[c][2] = q[1];
          raw[c][3] = q[WRP + 1];
        }
        MODE_SB
        MODE_MFH(0, b1, 0) hsplit(2); MODE_SB
        MODE_MFH(0, b1, 1) hsplit(3); MODE_SB
        opw[0] = make_uint4(q1[0], q1[1], q1[2], q1[3]);
        opw[64] = make_uint4(q2[0], q2[1], q2[2], q2[3]);
        if (k < 4) {
          issue(chn, 2 * k, 2 * k);
          issue(chn, 2 * k + 1, 2 * k + 1);
        }
        MODE_SB
        MODE_MFH(0, b1, 2) MODE_SB
        if (k >= STAGE_LAG && k < 4 + STAGE_LAG) commit(chn, 2 * (k - STAGE_LAG), 2 * (k - STAGE_LAG), nxt);
        MODE_SB
        MODE_MFH(0, b1, 3) MODE_SB
        if (k >= STAGE_LAG && k < 4 + STAGE_LAG) commit(chn, 2 * (k - STAGE_LAG) + 1, 2 * (k - STAGE_LAG) + 1, nxt);
        MODE_SB
#pragma unroll
        for (int p = 0; p < 2; ++p) acur[p] = anxt[p];
#pragma unroll
        for (int gi = 0; gi < 4; ++gi) b0[gi] = b0n[gi];
        lds_barrier();
      }
    }
  } else {

  for (int ch = 0; ch < NCH16; ++ch) {
    float* cur = smem + (ch & 1) * SP_WIN;
    float* nxt = smem + ((ch + 1) & 1) * SP_WIN;
    const int chn = ch + 1 < NCH16 ? ch + 1 : ch;  // (after the last chunk the same window is staged again: no branch in the body)
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      const int step = ch * KT + k;
      const int nstep = step + 1 < nsteps ? step + 1 : nsteps - 1;
      const int ks = (k + 2) % KT;                          // the tap that is sampled under this one
      const float* wsrc = k + 2 < KT ? cur : nxt;           // (taps 0, 1 of the next chunk: its window is complete since tap 5)
      const uint4* fcur = fragbase + (k % 3) * SP_OP;       // (9 taps per chunk: step % 3 == k % 3)
      const uint4* fnxt = fragbase + ((k + 1) % 3) * SP_OP;
      uint4* opw = opbuf + ((k + 2) % 3) * SP_OP + (wave * 3) * 64 + lane;
      const float4 tw = rw[ks];
      const float* wp_ = wsrc + half * 8 * CP + roff[ks];
      // (the first half batch of the NEXT tap's sampling is requested in slot 20 of this one: read at the top of its own tap, the
      // first combine waited for it right behind the barrier, with both waves of a SIMD in the same place)
      const float* wpn_ = (k + 3 < KT ? cur : nxt) + half * 8 * CP + roff[(k + 3) % KT];
      auto words = [&](const float* wp, int hb) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float* q = wp + (hb * 4 + c) * CP;
          raw[c][0] = q[0];
          raw[c][1] = q[WRP];
          raw[c][2] = q[1];
          raw[c][3] = q[WRP + 1];
        }
      };
      auto combine = [&](int c) {  // (one fma chain per value, kept scalar: see split3_bf16_pinned)
        v[c] = __builtin_fmaf(tw.w, raw[c & 3][3], __builtin_fmaf(tw.z, raw[c & 3][2], __builtin_fmaf(tw.y, raw[c & 3][1], tw.x * raw[c & 3][0])));
        asm("" : "+v"(v[c]));
      };
      auto split_a = [&](int j) {
        ra[j] = v[2 * j];
        rb[j] = v[2 * j + 1];
        q1[j] = split_step_bf16_pinned(ra[j], rb[j]);
      };
      auto split_b = [&](int j) { q2[j] = split_step_bf16_pinned(ra[j], rb[j]); };
      auto split_c = [&](int j) { q3[j] = pack2(ra[j], rb[j]); };

      // top of the tap: weight fragments of the next tap (global), the first half batch of window words
#pragma unroll
      for (int p = 0; p < 3; ++p) anxt[p] = (wpa + (long long)nstep * MTW * 192)[(unsigned)(p * 64 + lane)];
      MODE_SB
      MODE_MF(2, b0, 0) combine(0); MODE_SB
      MODE_MF(2, b0, 1) combine(1); MODE_SB
      MODE_MF(2, b0, 2) combine(2); MODE_SB
      MODE_MF(2, b0, 3) combine(3); MODE_SB
      words(wp_, 1);
#pragma unroll
      for (int gi = 0; gi < 4; ++gi) b1[gi] = fcur[(gi * 3 + 1) * 64];
      MODE_SB
      MODE_MF(1, b0, 0) split_a(0); MODE_SB
      MODE_MF(1, b0, 1) split_b(0); MODE_SB
      MODE_MF(1, b0, 2) split_c(0); split_a(1); MODE_SB
      MODE_MF(1, b0, 3) split_b(1); MODE_SB
      MODE_MF(0, b0, 0) split_c(1); combine(4); MODE_SB
      MODE_MF(0, b0, 1) combine(5); MODE_SB
      MODE_MF(0, b0, 2) combine(6); MODE_SB
      MODE_MF(0, b0, 3) combine(7); MODE_SB
#pragma unroll
      for (int gi = 0; gi < 4; ++gi) b2[gi] = fcur[(gi * 3 + 2) * 64];
      MODE_SB
      MODE_MF(1, b1, 0) split_a(2); MODE_SB
      MODE_MF(1, b1, 1) split_b(2); MODE_SB
      MODE_MF(1, b1, 2) split_c(2); split_a(3); MODE_SB
      MODE_MF(1, b1, 3) split_b(3); MODE_SB
      MODE_MF(0, b1, 0) split_c(3); MODE_SB
      opw[0] = make_uint4(q1[0], q1[1], q1[2], q1[3]);
      opw[64] = make_uint4(q2[0], q2[1], q2[2], q2[3]);
      opw[128] = make_uint4(q3[0], q3[1], q3[2], q3[3]);
      MODE_SB
      MODE_MF(0, b1, 1) MODE_SB
      // window of the next chunk: two phases loaded under each of taps 0..3, stored STAGE_LAG taps later (the whole window is in LDS
      // before tap 7 samples from it)
      if (k < 4) {
        issue(chn, 2 * k, 2 * k);
        issue(chn, 2 * k + 1, 2 * k + 1);
      }
      MODE_SB
      MODE_MF(0, b1, 2) MODE_SB
      MODE_MF(0, b1, 3) MODE_SB
#pragma unroll
      for (int gi = 0; gi < 4; ++gi) b0n[gi] = fnxt[(gi * 3 + 0) * 64];
      words(wpn_, 0);
      MODE_SB
      MODE_MF(0, b2, 0) MODE_SB
      if (k >= STAGE_LAG && k < 4 + STAGE_LAG) commit(chn, 2 * (k - STAGE_LAG), 2 * (k - STAGE_LAG), nxt);
      MODE_SB
      MODE_MF(0, b2, 1) MODE_SB
      if (k >= STAGE_LAG && k < 4 + STAGE_LAG) commit(chn, 2 * (k - STAGE_LAG) + 1, 2 * (k - STAGE_LAG) + 1, nxt);
      MODE_SB
      MODE_MF(0, b2, 2) MODE_SB
      MODE_MF(0, b2, 3) MODE_SB
#pragma unroll
      for (int p = 0; p < 3; ++p) acur[p] = anxt[p];
#pragma unroll
      for (int gi = 0; gi < 4; ++gi) b0[gi] = b0n[gi];
      lds_barrier();
    }
  }
  }
  MODE_STAMP(2)

  // D[i = o][j = pixel of group gset + gi]
  const int hh = h0 + (wave / TW) * 32 + (lane & 31);
  const int cmax = d.Cog - mg * 128;
  // eval mode: the 16 folded-BatchNorm shifts of this lane's output channels, ONCE (the same for the four pixel groups): read inside the
  // store loop every store waited for a load of its own -- `shift` may alias y as far as the compiler knows (round 5, ISA scan: 256
  // `s_waitcnt vmcnt(0)` in this kernel)
  float shv[16];
  if (EPI) {
#pragma unroll
    for (int r = 0; r < 16; ++r) shv[r] = epi.shift[g * d.Cog + mg * 128 + min(MODE_ACC_ROW(m, r, half), cmax - 1)];
  }
  const bool full_m = m * 32 + 32 <= cmax;  // (uniform per wave) every channel of this M-tile exists: no test per store
#pragma unroll
  for (int gi = 0; gi < 4; ++gi) {
    const int ww = w0 + gi;
    if (hh < d.H && ww < d.W) {
      float* yb = y + ((long long)b * d.Co + (long long)g * d.Cog + (long long)mg * 128) * HW + (long long)hh * d.sh + (long long)ww * d.sw;
      // eval mode: the residual values of this pixel group are requested together, ahead of its stores (`add` may alias `y` for all the
      // compiler knows: read next to the stores, each load waited for the store in front of it -- see deconv3d_kernel)
      float res[16];
      if (EPI) {
#pragma unroll
        for (int r = 0; r < 16; ++r) res[r] = 0.f;
        if (epi.add) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int co = min(MODE_ACC_ROW(m, r, half), cmax - 1);
            res[r] = epi.add[(yb - y) + (long long)co * HW];
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      auto emit = [&](int r) {
        const int co = MODE_ACC_ROW(m, r, half);
        if (EPI) {
          const float v = (acc[gi][r] + shv[r]) + res[r];
          yb[(long long)co * HW] = epi.relu ? relu_nan(v) : v;
        } else {
          yb[(long long)co * HW] = F16 ? acc[gi][r] * unscale : acc[gi][r];
        }
      };
      if (full_m) {
#pragma unroll
        for (int r = 0; r < 16; ++r) emit(r);
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (MODE_ACC_ROW(m, r, half) < cmax) emit(r);
      }
      if (EPI) __builtin_amdgcn_sched_barrier(0);
    }
  }
  MODE_STAMP(3)
}

}  // namespace

extern "C" size_t mode_sphere_conv_win_wpack_bytes(int Ci, int Co, int Kh, int Kw, int groups) {
  if (Ci <= 0 || Co <= 0 || groups <= 0 || Kh * Kw != KT || Ci % groups || Co % groups) return 0;
  const int Cig = Ci / groups, Cog = Co / groups;
  const size_t f32 = (size_t)groups * mode::cdiv(Cog, 128) * mode::cdiv(Cig, CCH) * KT * MTW * 64 * 4 + (size_t)Co;  // + shifts
  const size_t split = (size_t)groups * mode::cdiv(Cog, 128) * mode::cdiv(Cig, SP_CCH) * KT * MTW * 3 * 64 * 4;       // split-bf16 fragments
  const size_t tall = (size_t)groups * mode::cdiv(Cog, 128) * mode::cdiv(Cig, CCH) * TP * MTW * 3 * 64 * 4;            // ... of the tall tiles
  return (((f32 + 3) / 4) * 4 + split + tall) * sizeof(float);
}

namespace {
template <bool EPI>
int fwd_win_launch(const float* x, const float* pos, float* y, const float* wpack, const int32_t* tiles, int n_small, int n_mid,
                   int n_wrap, int B, const WinDims& d, hipStream_t st, const Epi& epi);
}

static int sphere_conv_fwd_win_impl(const float* x, const float* pos, const float* w, float* y, float* wpack, const int32_t* tiles,
                                    int n_small, int n_mid, int n_wrap, int B, int Ci, int H, int W, int Co, int Kh, int Kw, int groups,
                                    int transposed, mode_stream_t stream, const mode_bn_epilogue* bn, int split = 0,
                                    const float* amax_x = nullptr, const float* amax_w = nullptr) {
  WinDims d;
  int rc = make_win_dims(d, B, Ci, H, W, Co, Kh, Kw, groups, "mode_sphere_conv_fwd_win");
  MODE_REQUIRE((amax_x == nullptr) == (amax_w == nullptr) && !(amax_x && bn), MODE_ERR_BAD_ARG,
               "mode_sphere_conv_fwd_win: the fp16 arithmetic takes both operand maxima and no BatchNorm epilogue");
  const bool f16 = amax_x != nullptr;
  if (rc != MODE_OK) return rc;
  if (transposed) {
    d.sh = 1;
    d.sw = H;
  }
  MODE_REQUIRE(n_small >= 0 && n_mid >= 0 && n_wrap >= 0 && (size_t)n_small + n_mid + n_wrap == mode_sphere_plan_max_tiles(H, W),
               MODE_ERR_BAD_ARG, "mode_sphere_conv_fwd_win: the plan must cover every tile (%d + %d + %d given, %zu tiles)", n_small, n_mid,
               n_wrap, mode_sphere_plan_max_tiles(H, W));
  if (B == 0) return MODE_OK;
  MODE_REQUIRE(x && pos && w && y && wpack && tiles, MODE_ERR_BAD_ARG, "mode_sphere_conv_fwd_win: null pointer");
  MODE_REQUIRE(B <= 65535 && d.G * d.MG <= 65535, MODE_ERR_UNSUPPORTED, "mode_sphere_conv_fwd_win: grid limit");
  hipStream_t st = mode::as_stream(stream);
  const long long npack = (long long)d.G * d.MG * d.NCH * KT * MTW * 64 * 4;
  const bool split_path = split && n_small > 0 && d.Cig % SP_CCH == 0;
  const bool wrap_on_fp32 = n_wrap > 0 && (!d.wrap_pipe || tall_split_lds_bytes(d.wr) > 160 * 1024);
  // the fp32 fragment layout (and the folded-BatchNorm shifts behind it) is read by the fp32 kernels and by the eval epilogue: a training
  // call whose tiles all run on the split kernel does not need it
  if (mode::pack_needed() && (!split_path || bn || wrap_on_fp32))
    hipLaunchKernelGGL(pack_w_win, dim3(mode::cdiv(npack, 256)), dim3(256), 0, st, w, wpack, d, bn ? 1 : 0, bn ? *bn : mode_bn_epilogue());
  const Epi epi = make_epi(bn, wpack + npack);
  if (split_path) {
    // ALL window classes on the split kernel, in the arithmetic of the entry (three bf16 pieces, or two fp16 pieces: the tall-window
    // tiles too, pack_w_win_split_tall<f16>) -- but for wrap-around tiles that cannot be double-buffered (wrap_on_fp32: fp32 kernel)
    const int NCH16 = d.Cig / SP_CCH;
    uint4* wps = reinterpret_cast<uint4*>(wpack + ((npack + d.Co + 3) / 4) * 4);
    const long long nsplit = (long long)d.G * d.MG * NCH16 * KT * MTW * 64;
    // (the fp16 arithmetic comes without an epilogue: fold = 0 there, and amax_w is null on three bf16 pieces)
    const int fold = bn ? 1 : 0;
    const mode_bn_epilogue fbn = bn ? *bn : mode_bn_epilogue();
    if (mode::pack_needed())
      hipLaunchKernelGGL((f16 ? pack_w_win_split<true> : pack_w_win_split<false>), dim3(mode::cdiv(nsplit, 256)), dim3(256), 0, st, w, wps, d,
                         NCH16, fold, fbn, amax_w);
    uint4* wpt = wps + nsplit * 3;  // fragments of the tall-window tiles: K = 8 channels x 2 taps
    if (n_mid + n_wrap > 0 && mode::pack_needed()) {
      const long long ntall = (long long)d.G * d.MG * d.NCH * TP * MTW * 64;
      hipLaunchKernelGGL((f16 ? pack_w_win_split_tall<true> : pack_w_win_split_tall<false>), dim3(mode::cdiv(ntall, 256)), dim3(256), 0, st, w,
                         wpt, d, fold, fbn, amax_w);
    }
    // one launch for all tiles; wrap-around tiles that cannot be double-buffered keep their own kernel
    const int4* tl = reinterpret_cast<const int4*>(tiles);
    int n_all = n_small + n_mid + n_wrap;
    if (wrap_on_fp32) {
      rc = bn ? fwd_win_launch<true>(x, pos, y, wpack, tiles, 0, 0, n_wrap, B, d, st, epi)
              : fwd_win_launch<false>(x, pos, y, wpack, tiles, 0, 0, n_wrap, B, d, st, epi);
      if (rc != MODE_OK) return rc;
      tl += n_wrap;
      n_all -= n_wrap;
      n_wrap = 0;
    }
    size_t lds = SP3_LDS_BYTES;
    if (n_mid > 0) lds = std::max(lds, tall_split_lds_bytes(WR_MID));
    if (n_wrap > 0) lds = std::max(lds, tall_split_lds_bytes(d.wr));
    auto run = [&](auto kernel) {
      return launch_win("mode_sphere_conv_fwd_win_split", kernel, dim3(n_all, B, d.G * d.MG), lds, st, x, pos, wps, wpt, y, d, NCH16, tl, epi,
                        amax_x, amax_w);
    };
    return bn ? run(sphere_fwd_split_kernel<true>) : f16 ? run(sphere_fwd_split_kernel<false, true>) : run(sphere_fwd_split_kernel<false>);
  }
  return bn ? fwd_win_launch<true>(x, pos, y, wpack, tiles, n_small, n_mid, n_wrap, B, d, st, epi)
            : fwd_win_launch<false>(x, pos, y, wpack, tiles, n_small, n_mid, n_wrap, B, d, st, epi);
}

namespace {
template <bool EPI>
int fwd_win_launch(const float* x, const float* pos, float* y, const float* wpack, const int32_t* tiles, int n_small, int n_mid,
                   int n_wrap, int B, const WinDims& d, hipStream_t st, const Epi& epi) {
  // tile list order: wrap-around tiles, then mid, then small
  const float4* wp4 = reinterpret_cast<const float4*>(wpack);
  const int4* tl = reinterpret_cast<const int4*>(tiles);
  int n_main = n_small + n_mid + n_wrap;
  int rc = MODE_OK;
  if (n_wrap > 0 && !d.wrap_pipe) {
    rc = launch_win("mode_sphere_conv_fwd_win", sphere_fwd_win_tall_kernel<EPI>, dim3(n_wrap, B, d.G * d.MG), win_lds_bytes(d.wr, false), st, x,
                    pos, wp4, y, d, tl, epi);
    if (rc != MODE_OK) return rc;
    tl += n_wrap;
    n_main -= n_wrap;
    n_wrap = 0;
  }
  if (n_main > 0) {
    size_t lds = 0;
    if (n_small > 0) lds = std::max(lds, win_lds_bytes(WR_SMALL, true));
    if (n_mid > 0) lds = std::max(lds, win_lds_bytes(WR_MID, true));
    if (n_wrap > 0) lds = std::max(lds, win_lds_bytes(d.wr, true));
    rc = launch_win("mode_sphere_conv_fwd_win", sphere_fwd_win_kernel<EPI>, dim3(n_main, B, d.G * d.MG), lds, st, x, pos, wp4, y, d, tl, epi);
  }
  return rc;
}
}  // namespace

extern "C" int mode_sphere_conv_fwd_win(const float* x, const float* pos, const float* w, float* y, float* wpack,
                                        const int32_t* tiles, int n_small, int n_mid, int n_wrap, int B, int Ci, int H, int W, int Co,
                                        int Kh, int Kw, int groups, int transposed, mode_stream_t stream) {
  return sphere_conv_fwd_win_impl(x, pos, w, y, wpack, tiles, n_small, n_mid, n_wrap, B, Ci, H, W, Co, Kh, Kw, groups, transposed, stream,
                                  nullptr);
}

// Small-window tiles on the split-bf16 matrix path (sphere_fwd_split_kernel), the other classes on the fp32 kernels; bn may be NULL.
extern "C" int mode_sphere_conv_fwd_win_split(const float* x, const float* pos, const float* w, const mode_bn_epilogue* bn, float* y,
                                              float* wpack, const int32_t* tiles, int n_small, int n_mid, int n_wrap, int B, int Ci, int H,
                                              int W, int Co, int Kh, int Kw, int groups, int transposed, mode_stream_t stream) {
  if (bn) {
    int rc = mode::check_bn(bn, "mode_sphere_conv_fwd_win_split");
    if (rc != MODE_OK) return rc;
  }
  return sphere_conv_fwd_win_impl(x, pos, w, y, wpack, tiles, n_small, n_mid, n_wrap, B, Ci, H, W, Co, Kh, Kw, groups, transposed, stream, bn,
                                  1);
}

// The training forward with the small-window tiles on the two-piece fp16 arithmetic: amax_x / amax_w = device scalars holding the largest
// finite magnitude of x and of w (mode_abs_max, or the BatchNorm pass that wrote x).  Same results contract as the split-bf16 entry.
extern "C" int mode_sphere_conv_fwd_win_split_f16(const float* x, const float* pos, const float* w, const float* amax_x, const float* amax_w,
                                                  float* y, float* wpack, const int32_t* tiles, int n_small, int n_mid, int n_wrap, int B,
                                                  int Ci, int H, int W, int Co, int Kh, int Kw, int groups, int transposed,
                                                  mode_stream_t stream) {
  MODE_REQUIRE(amax_x && amax_w, MODE_ERR_BAD_ARG, "mode_sphere_conv_fwd_win_split_f16: null maximum");
  return sphere_conv_fwd_win_impl(x, pos, w, y, wpack, tiles, n_small, n_mid, n_wrap, B, Ci, H, W, Co, Kh, Kw, groups, transposed, stream,
                                  nullptr, 1, amax_x, amax_w);
}

extern "C" int mode_sphere_conv_fwd_win_bn(const float* x, const float* pos, const float* w, const mode_bn_epilogue* bn, float* y,
                                           float* wpack, const int32_t* tiles, int n_small, int n_mid, int n_wrap, int B, int Ci, int H,
                                           int W, int Co, int Kh, int Kw, int groups, int transposed, mode_stream_t stream) {
  int rc = mode::check_bn(bn, "mode_sphere_conv_fwd_win_bn");
  if (rc != MODE_OK) return rc;
  return sphere_conv_fwd_win_impl(x, pos, w, y, wpack, tiles, n_small, n_mid, n_wrap, B, Ci, H, W, Co, Kh, Kw, groups, transposed, stream, bn);
}

#ifdef MODE_TAPTIME
namespace {
__global__ void taptime_copy_kernel(unsigned long long* out, int n) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = g_taptime[i];
}
}  // namespace
extern "C" int mode_debug_taptime(unsigned long long* dev_out, int n) {
  hipLaunchKernelGGL(taptime_copy_kernel, dim3(64), dim3(256), 0, 0, dev_out, n);
  return (int)hipDeviceSynchronize();
}
#endif
