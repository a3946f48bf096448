// Spherical convolution, "windowed" weight-gradient kernels for gfx950 (MI355X): the compact-window tiles and the polar items, each
// on fp32 MFMAs and on the split arithmetic of split_arith.h, and the fixed-order reduction of their partial sums.
// sphere_win_internal.h says what a window is and who plans the tiles.
#include "sphere_win_internal.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// Backward w.r.t. the weight on the compact-window tiles:  gW[o][c][k] = sum_p gy[o][p] * col[c][k][p]
//   D[i = o][j = c] per tap, K = the pixels of the tile; A = gy (LDS, [o][pixel]), B = col built on the fly from the x window
//   of 32 input channels (LDS, [c][col][row], odd channel pitch: the 32 lanes of a half-wave read 32 channels).
// Work item = half a plan tile (32 rows x 4 columns) of one sample, processed column by column (32 pixels = 16 k-steps).
// grid = (S, ceil(Cig/32), G*MG); split-K slice s owns the items s, s+S, ...; 8 waves: wave v owns tap v for all 4 o-tiles,
// tap 8 is shared: wave v takes the pixels p = v (mod 8) of every column (the 8 shares are summed through LDS in wave order
// at the end).  Partial sums go to part[s][z][cg][tap][128 o][32 c], summed in fixed order by reduce_gw_win.
// The contraction runs on v_mfma_f32_32x32x1_2b_f32: ONE pixel per instruction, two o-tiles (the two 32x32 blocks) at a time.
// With one pixel per step the sampling record is the same for the whole wave, so it lives in SGPRs (scalar loads from the
// record table) and the bilinear combine is 4 VALU instructions with scalar weights -- the 32x32x2 form (two pixels per step,
// one per half-wave) needed ~14 VALU + 7 SALU instructions per MFMA for the per-half selects and measured 30 % MFMA busy.
// The sampling records (window offset + 4 weights per tap and pixel) come from a table the host builds with the plan
// (mode_sphere_plan_records): they depend on the table and the tile only, not on the sample, layer or channel group.
// Everything the next column needs (gy, records; the x window before a new item) is fetched into registers before the MFMAs
// of the current column and written to the other LDS buffer after them.
constexpr int BW_CG = 32;
constexpr int BW_CP = WC * BW_WR + 1;      // odd channel pitch of the x window
constexpr int BW_GP = BW_TH + 1;           // gy row pitch
constexpr int BW_SLOTS = KT;                // one partial per tap (the waves' shares of tap 8 are summed in the kernel)
constexpr int BW_XW = BW_CG * BW_CP + BW_WR + 8;  // + slack: zero-weight corners may point just past the last window
constexpr int BW_COLBUF = 128 * BW_GP;  // gy column
constexpr int BW_LDS_FLOATS = 2 * BW_XW + 2 * BW_COLBUF;  // x window and gy column, both double-buffered
constexpr int BW_NXW = BW_CG / TW;  // x-window words per thread and column step: the next item's window arrives in 4 parts

// The 72 MFMAs of one column (32 pixels) of a work item for this wave: own tap (all 32 pixels, software-pipelined: while the
// MFMAs of pixel px run, the B value of pixel px+1 is combined and the LDS words of pixel px+2 are requested), then this wave's
// share of tap 8.  cb = gy column [128][BW_GP], xw = x window(s) [32][CP], rw/ro (rw8/ro8) = lane l holds the record of pixel
// l & 31 of this wave's tap (of tap 8); WRP = distance between the two window columns of a record.
template <int WRP, int CP>
__device__ __forceinline__ void bww_column(const float* cb, const float* xw, const float4 rw, const int ro, const float4 rw8,
                                           const int ro8, f32x32 (&accp)[2], f32x32 (&acc8p)[2], int wave_u, int j, int half) {
  // A operand: block 0 (lanes 0-31) = o-tile 0 / 2, block 1 (lanes 32-63) = o-tile 1 / 3
  const float* ap = cb + (half * 32 + j) * BW_GP;
  const float* xb = xw + j * CP;
  auto load_x = [&](int o, float (&raw)[4]) {  // o is wave-uniform
    const float* p = xb + o;
    raw[0] = p[0];
    raw[1] = p[WRP];
    raw[2] = p[1];
    raw[3] = p[WRP + 1];
  };
  auto bcast = [&](float v, int px) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), px)); };
  auto combine = [&](const float4& w, int px, const float (&raw)[4]) {  // one fma chain: keeps the compiler from SLP-packing
    return __builtin_fmaf(bcast(w.w, px), raw[3],
                          __builtin_fmaf(bcast(w.z, px), raw[2], __builtin_fmaf(bcast(w.y, px), raw[1], bcast(w.x, px) * raw[0])));
  };
  // own tap: all 32 pixels, software-pipelined three deep: while the MFMAs of pixel px run, the B value of pixel px+1 is
  // combined (4 FMAs on words read one step earlier) and the LDS words of pixel px+2 are requested
  {
    float raw[2][4], a[3][2];
#pragma unroll
    for (int p0 = 0; p0 < 2; ++p0) {
      load_x(__builtin_amdgcn_readlane(ro, p0), raw[p0]);
      a[p0][0] = ap[p0];
      a[p0][1] = ap[64 * BW_GP + p0];
    }
    float bv = combine(rw, 0, raw[0]);
#pragma unroll
    for (int px = 0; px < BW_TH; ++px) {
      const int c3 = px % 3, n3 = (px + 2) % 3;
      float bv_next = 0.f;
      if (px + 1 < BW_TH) bv_next = combine(rw, px + 1, raw[(px + 1) & 1]);
      if (px + 2 < BW_TH) {
        load_x(__builtin_amdgcn_readlane(ro, px + 2), raw[px & 1]);  // the slot of pixel px is free again
        a[n3][0] = ap[px + 2];
        a[n3][1] = ap[64 * BW_GP + px + 2];
      }
      __builtin_amdgcn_sched_barrier(0);
      accp[0] = __builtin_amdgcn_mfma_f32_32x32x1f32(a[c3][0], bv, accp[0], 0, 0, 0);
      accp[1] = __builtin_amdgcn_mfma_f32_32x32x1f32(a[c3][1], bv, accp[1], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      bv = bv_next;
    }
  }
  // this wave's share of tap 8: pixels wave, wave + 8, wave + 16, wave + 24
  {
    float raw[4][4], a[4][2];
#pragma unroll
    for (int i = 0; i < BW_TH / 8; ++i) {
      const int px = wave_u + 8 * i;
      load_x(__builtin_amdgcn_readlane(ro8, px), raw[i]);
      a[i][0] = ap[px];
      a[i][1] = ap[64 * BW_GP + px];
    }
#pragma unroll
    for (int i = 0; i < BW_TH / 8; ++i) {
      const float b8 = combine(rw8, wave_u + 8 * i, raw[i]);
      acc8p[0] = __builtin_amdgcn_mfma_f32_32x32x1f32(a[i][0], b8, acc8p[0], 0, 0, 0);
      acc8p[1] = __builtin_amdgcn_mfma_f32_32x32x1f32(a[i][1], b8, acc8p[1], 0, 0, 0);
    }
  }

}

// Partials of one workgroup: tap `wave` from its wave, tap 8 = the 8 waves' shares added in wave order through LDS (deterministic).
// Must be called after a barrier that ends all reads of `smem`.
__device__ __forceinline__ void bww_write_partials(float* pb, float* smem, f32x32 (&accp)[2], f32x32 (&acc8p)[2], int wave, int half,
                                                   int j, int tid) {
#pragma unroll
  for (int pr = 0; pr < 2; ++pr)
#pragma unroll
    for (int r = 0; r < 32; ++r) {
      const int o = (2 * pr + (r >> 4)) * 32 + (r & 3) + 8 * ((r & 15) >> 2) + 4 * half;
      pb[((long long)wave * 128 + o) * BW_CG + j] = accp[pr][r];
    }
  // tap 8: the 8 waves' shares, added in wave order through LDS (deterministic), then written as one partial
  float* red = smem;  // [128 o][32 c]; the item loop ended with a barrier, nobody reads the windows any more
  for (int v = 0; v < 8; ++v) {
    if (wave == v) {
#pragma unroll
      for (int pr = 0; pr < 2; ++pr)
#pragma unroll
        for (int r = 0; r < 32; ++r) {
          const int o = (2 * pr + (r >> 4)) * 32 + (r & 3) + 8 * ((r & 15) >> 2) + 4 * half;
          float* q = red + o * BW_CG + j;
          *q = v == 0 ? acc8p[pr][r] : *q + acc8p[pr][r];
        }
    }
    __syncthreads();
  }
  for (int i = tid; i < 128 * BW_CG; i += NTHREADS) pb[(long long)8 * 128 * BW_CG + i] = red[i];
}

__global__ __launch_bounds__(NTHREADS) void sphere_bww_win_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                                   float* __restrict__ part, WinDims d, const int4* __restrict__ tiles,
                                                                   const float4* __restrict__ rec_w, const int* __restrict__ rec_off,
                                                                   int ntiles, int S) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* colbuf = smem + 2 * BW_XW;  // smem: [2][x window 32 x BW_CP] [2][gy column]
  constexpr int WRP = BW_WR;
  const int s = blockIdx.x, cg = blockIdx.y;
  const int g = blockIdx.z / d.MG, mg = blockIdx.z % d.MG;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int j = lane & 31, half = lane >> 5;
  const long long HW = (long long)d.H * d.W;
  const int T = ntiles * 2 * d.B;  // (sample, tile, half) items
  const int NCG = gridDim.y;

  f32x32 accp[2], acc8p[2];  // [o-tile pair]: elements 0-15 = first tile of the pair, 16-31 = second
#pragma unroll
  for (int r = 0; r < 32; ++r) {
    accp[0][r] = accp[1][r] = 0.f;
    acc8p[0][r] = acc8p[1][r] = 0.f;
  }
  for (int i = tid; i < BW_LDS_FLOATS; i += NTHREADS) smem[i] = 0.f;  // every word that may be read is finite

  // prefetch registers
  float pxw[BW_NXW];  // x window of the next item
  float pgy[8];       // gy of the next column: o = (tid >> 5) + 16 u, pixel tid & 31
  float4 prw, prw8;   // records of the next column: lane l holds pixel l & 31 of this wave's tap and of tap 8
  int pro, pro8;

  const int omax = d.Cog - mg * 128;
  const int cmax = d.Cig - cg * BW_CG;
  const int gpx = tid & (BW_TH - 1), go0 = tid >> 5;

  struct Item {  // geometry of a work item, wave-uniform
    int b, ti, hf, h0, w0, rbase, cbase;
  };
  auto item_of = [&](int t) {
    Item it;
    it.b = t / (ntiles * 2);
    const int r = t - it.b * ntiles * 2;
    it.ti = r >> 1;
    it.hf = r & 1;
    const int4 tl = tiles[it.ti];
    it.h0 = tl.x + it.hf * BW_TH;
    it.w0 = tl.y;
    it.rbase = (tl.z + it.hf * BW_TH) % d.H;
    it.cbase = tl.w & 0xffff;
    return it;
  };
  // x window: thread -> (column, row < 49), one word per channel; addresses are base + channel * stride.  Lanes run along the
  // contiguous axis of the planes (columns for NCHW, rows for transposed planes).
  const int xcol = d.sh == 1 ? tid >> 6 : tid & (WC - 1), xrow = d.sh == 1 ? tid & 63 : tid >> 3;
  const bool xrow_ok = xrow < WRP;
  // Loads are issued unconditionally from clamped addresses and masked when they are written to LDS: a load whose only
  // consumer is a select on the same condition gets sunk into a branch by the compiler, with a full vmcnt(0) wait per load
  // (measured: 7.6k cycles per column spent "issuing" 12 loads).
  bool pxw_ok = false;   // row / column of this thread's window words inside the image (next item)
  unsigned pgy_ok = 0;   // bit u: pgy[u] is a real value (next column)
  auto issue_xw = [&](const Item& it, int part) {  // channels part*8 .. part*8+7 of the window of item `it`
    pxw_ok = xrow_ok && it.cbase + xcol < d.W;
    const int grow = (it.rbase + (xrow_ok ? xrow : 0)) % d.H;
    const float* xg = x + ((long long)it.b * d.Ci + (long long)g * d.Cig + (long long)cg * BW_CG) * HW +
                      (pxw_ok ? (long long)grow * d.sh + (long long)(it.cbase + xcol) * d.sw : 0);
#pragma unroll
    for (int c = 0; c < BW_NXW; ++c) pxw[c] = xg[(long long)min(part * BW_NXW + c, cmax - 1) * HW];
  };
  auto commit_xw = [&](float* xwdst, int part) {
    if (xrow_ok) {
      float* dst = xwdst + xcol * WRP + xrow;
#pragma unroll
      for (int c = 0; c < BW_NXW; ++c) dst[(part * BW_NXW + c) * BW_CP] = (pxw_ok && part * BW_NXW + c < cmax) ? pxw[c] : 0.f;
    }
  };
  auto issue_col = [&](const Item& it, int wc) {
    const int h = it.h0 + gpx, w = it.w0 + wc;
    const bool pok = h < d.H && w < d.W;
    const float* gyb = gy + ((long long)it.b * d.Co + (long long)g * d.Cog + (long long)mg * 128) * HW +
                       (pok ? (long long)h * d.sh + (long long)w * d.sw : 0);
    pgy_ok = 0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int o = go0 + 16 * u;
      pgy[u] = gyb[(long long)min(o, omax - 1) * HW];
      pgy_ok |= (pok && o < omax) ? (1u << u) : 0u;
    }
    const long long rcol = (((long long)it.ti * 2 + it.hf) * TW + wc) * BW_NREC;
    prw = rec_w[rcol + wave * BW_TH + j];
    pro = rec_off[rcol + wave * BW_TH + j];
    prw8 = rec_w[rcol + 8 * BW_TH + j];
    pro8 = rec_off[rcol + 8 * BW_TH + j];
  };
  auto commit_col = [&](float* cb) {
#pragma unroll
    for (int u = 0; u < 8; ++u) cb[(go0 + 16 * u) * BW_GP + gpx] = (pgy_ok >> u & 1u) ? pgy[u] : 0.f;
  };

  // first item: window and first column
  Item cur = item_of(s);
  __syncthreads();  // zero fill done
  for (int part = 0; part < TW; ++part) {
    issue_xw(cur, part);
    commit_xw(smem, part);
  }
  issue_col(cur, 0);
  commit_col(colbuf);
  __syncthreads();

  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  int buf = 0, xbuf = 0;
  for (int t = s; t < T; t += S) {
    const bool more_items = t + S < T;
    const Item nxt = item_of(more_items ? t + S : t);
    const float* xw = smem + xbuf * BW_XW;
    for (int wc = 0; wc < TW; ++wc) {
      const float* cb = colbuf + buf * BW_COLBUF;
      const bool last_col = wc == TW - 1;
      const bool have_next = !last_col || more_items;
      // The sampling record of a pixel is the same for every lane: lane l holds the record of pixel l & 31 (vector loads,
      // prefetched with the column) and each step broadcasts its pixel's record with v_readlane -- no scalar-memory loads
      // in the loop, whose out-of-order return would force a full LDS drain on every use.
      const float4 rw = prw, rw8 = prw8;
      const int ro = pro, ro8 = pro8;
      if (have_next) issue_col(last_col ? nxt : cur, last_col ? 0 : wc + 1);
      if (more_items) issue_xw(nxt, wc);  // a quarter of the next item's window per column, into the other window buffer

      bww_column<BW_WR, BW_CP>(cb, xw, rw, ro, rw8, ro8, accp, acc8p, wave_u, j, half);

      // the other buffers: nobody reads them now
      if (have_next) commit_col(colbuf + (buf ^ 1) * BW_COLBUF);
      if (more_items) commit_xw(smem + (xbuf ^ 1) * BW_XW, wc);
      __syncthreads();
      buf ^= 1;
    }
    cur = nxt;
    xbuf ^= 1;
  }

  bww_write_partials(part + ((((long long)s * gridDim.z + blockIdx.z) * NCG + cg) * BW_SLOTS) * (128 * BW_CG), smem, accp, acc8p, wave,
                     half, j, tid);
}

// ---------------------------------------------------------------------------------------------------------------------
// The same contraction for the tiles next to the poles, where the nine taps of one output column sample row ranges that lie far
// apart (so no single compact window exists): a work item is ONE column of 32 pixels, and the x window is nine small windows,
// one per tap: [32 ch][9 taps][2 columns][34 rows] (78 KB).  Everything of an item is staged in place (no cross-item prefetch:
// these items are 12.5 % of the pixels), then the k-loop of the compact-window kernel runs unchanged on it.
// pitems[i] = (h0, w, rbase[9], cbase[9]); records [item][tap][32] hold offsets into the per-tap layout.
constexpr int BP_CP = KT * BP_TAPW + 1;  // odd channel pitch (613)
constexpr int BP_XW = BW_CG * BP_CP + BP_WR + 8;
constexpr int BP_LDS_FLOATS = BP_XW + BW_COLBUF;

__global__ __launch_bounds__(NTHREADS) void sphere_bww_polar_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                                     float* __restrict__ part, WinDims d, const int* __restrict__ pitems,
                                                                     const float4* __restrict__ rec_w, const int* __restrict__ rec_off,
                                                                     int nitems, int S, int s_base) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* xw = smem;
  float* cb = smem + BP_XW;
  const int s = blockIdx.x, cg = blockIdx.y;
  const int g = blockIdx.z / d.MG, mg = blockIdx.z % d.MG;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int j = lane & 31, half = lane >> 5;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const long long HW = (long long)d.H * d.W;
  const int T = nitems * d.B;
  const int omax = d.Cog - mg * 128, cmax = d.Cig - cg * BW_CG;
  const int gpx = tid & (BW_TH - 1), go0 = tid >> 5;

  f32x32 accp[2], acc8p[2];
#pragma unroll
  for (int r = 0; r < 32; ++r) {
    accp[0][r] = accp[1][r] = 0.f;
    acc8p[0][r] = acc8p[1][r] = 0.f;
  }
  for (int i = tid; i < BP_LDS_FLOATS; i += NTHREADS) smem[i] = 0.f;

  // this thread's window words: element e = tid (and tid + 512 < 612) of the [9][2][34] per-channel layout
  constexpr int NE = KT * BP_TAPW;  // 612
  const int e0 = tid, e1 = tid + NTHREADS;
  const bool has1 = e1 < NE;
  const int k0 = e0 / BP_TAPW, k1 = (has1 ? e1 : 0) / BP_TAPW;
  const int col0 = (e0 % BP_TAPW) / BP_WR, r0 = e0 % BP_WR;
  const int col1 = ((has1 ? e1 : 0) % BP_TAPW) / BP_WR, r1 = (has1 ? e1 : 0) % BP_WR;

  for (int t = s; t < T; t += S) {
    const int b = t / nitems, it = t - b * nitems;
    const int* pi = pitems + (long long)it * BP_ITEM_INTS;
    const int h0 = pi[0], w = pi[1];
    __syncthreads();  // previous item consumed (first pass: zero fill done)
    {
      const int rb0 = pi[2 + k0], cb0 = pi[2 + KT + k0], rb1 = pi[2 + k1], cb1 = pi[2 + KT + k1];
      const bool ok0 = cb0 + col0 < d.W, ok1 = has1 && cb1 + col1 < d.W;
      const float* xg = x + ((long long)b * d.Ci + (long long)g * d.Cig + (long long)cg * BW_CG) * HW;
      const long long a0 = ok0 ? (long long)((rb0 + r0) % d.H) * d.sh + (long long)(cb0 + col0) * d.sw : 0;
      const long long a1 = ok1 ? (long long)((rb1 + r1) % d.H) * d.sh + (long long)(cb1 + col1) * d.sw : 0;
#pragma unroll 1
      for (int c8 = 0; c8 < BW_CG; c8 += 8) {  // 16 unconditional loads in flight, masked at the store
        float v0[8], v1[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const long long co = (long long)min(c8 + c, cmax - 1) * HW;
          v0[c] = xg[co + a0];
          v1[c] = xg[co + a1];
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          xw[(c8 + c) * BP_CP + e0] = (ok0 && c8 + c < cmax) ? v0[c] : 0.f;
          if (has1) xw[(c8 + c) * BP_CP + e1] = (ok1 && c8 + c < cmax) ? v1[c] : 0.f;
        }
      }
    }
    {
      const int h = h0 + gpx;
      const bool pok = h < d.H && w < d.W;
      const float* gyb = gy + ((long long)b * d.Co + (long long)g * d.Cog + (long long)mg * 128) * HW +
                         (pok ? (long long)h * d.sh + (long long)w * d.sw : 0);
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = gyb[(long long)min(go0 + 16 * u, omax - 1) * HW];
#pragma unroll
      for (int u = 0; u < 8; ++u) cb[(go0 + 16 * u) * BW_GP + gpx] = (pok && go0 + 16 * u < omax) ? v[u] : 0.f;
    }
    const long long rbase = (long long)it * BW_NREC;
    const float4 rw = rec_w[rbase + wave * BW_TH + j], rw8 = rec_w[rbase + 8 * BW_TH + j];
    const int ro = rec_off[rbase + wave * BW_TH + j], ro8 = rec_off[rbase + 8 * BW_TH + j];
    __syncthreads();
    bww_column<BP_WR, BP_CP>(cb, xw, rw, ro, rw8, ro8, accp, acc8p, wave_u, j, half);
  }
  __syncthreads();
  bww_write_partials(part + ((((long long)(s_base + s) * gridDim.z + blockIdx.z) * gridDim.y + cg) * BW_SLOTS) * (128 * BW_CG), smem, accp,
                     acc8p, wave, half, j, tid);
}

// gw[o][c][k] += sum over slices (fixed order) of the tap's partial; one thread per (z, cg, k, o, c), c fastest:
// coalesced reads of the partials
__global__ void reduce_gw_win(const float* __restrict__ part, float* __restrict__ gw, WinDims d, int S, int NCG) {
  const int GZ = d.G * d.MG;
  const long long total = (long long)GZ * NCG * KT * 128 * BW_CG;
  const long long stride = (long long)GZ * NCG * BW_SLOTS * 128 * BW_CG;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    const int cl = (int)(idx % BW_CG);
    long long r = idx / BW_CG;
    const int row = (int)(r % 128);
    r /= 128;
    const int k = (int)(r % KT);
    r /= KT;
    const int cg = (int)(r % NCG);
    const int z = (int)(r / NCG);
    const int g = z / d.MG, mg = z % d.MG;
    const int ol = mg * 128 + row, c = cg * BW_CG + cl;
    if (ol >= d.Cog || c >= d.Cig) continue;
    const float* pp = part + ((((long long)z * NCG + cg) * BW_SLOTS + k) * 128 + row) * BW_CG + cl;
    // fixed association (4 interleaved running sums over the slices): deterministic, 4 independent loads in flight
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int e = 0;
    for (; e + 3 < S; e += 4) {
      a0 += pp[(long long)e * stride];
      a1 += pp[(long long)(e + 1) * stride];
      a2 += pp[(long long)(e + 2) * stride];
      a3 += pp[(long long)(e + 3) * stride];
    }
    for (; e < S; ++e) a0 += pp[(long long)e * stride];
    const float sum = (a0 + a1) + (a2 + a3);
    gw[((long long)(g * d.Cog + ol) * d.Cig + c) * KT + k] += sum;
  }
}

int bww_win_splits(const WinDims& d, int ntiles) {
  const int T = ntiles * 2 * d.B;
  const int wgs_per_slice = mode::cdiv(d.Cig, BW_CG) * d.G * d.MG;
  const int per = std::max(1, mode::cdiv((long long)T * wgs_per_slice, kNumCU));  // items per workgroup for ~one workgroup per CU
  return std::max(1, mode::cdiv(T, per));
}

// =====================================================================================================================
// Weight gradient on the compact-window tiles with the split-bf16 arithmetic:  gW[o][c][k] = sum_p gy[o][p] * col[c][k][p],
// D[i = o][j = c] per tap on v_mfma_f32_32x32x16_bf16 with K = 16 PIXELS per instruction (sphere_bww_win_kernel: one pixel per fp32
// MFMA).  Same work items (half a plan tile = 32 rows x 4 columns of one sample, column by column), x window, record table, wave roles
// (wave v owns tap v for all four o-tiles; tap 8 is shared), partial-sum layout and reduction as sphere_bww_win_kernel.  New:
//   * gy is split when a column is staged: LDS holds [3 pieces][128 o][32 px] bf16 (row pitch 80 B: the 16 lanes of a b128 read
//     group hit 16 different 16-byte slots), so an A fragment (lane = o, 8 consecutive pixels) is ONE ds_read_b128 per piece;
//   * the B fragment (lane = c, 8 consecutive pixels) needs the sampled values pixel-fastest per channel, while sampling wants one
//     pixel per lane (its record in registers).  So a wave samples 16 pixels x 32 channels per K-step with lane = (pixel octet h,
//     channel octet q, pixel p8): 8 channels x (4 window words + 4 FMAs) for ITS pixel, transposes the 8 x 8 blocks through a
//     wave-private LDS scratch (8 ds_write_b32 + 8 ds_read_b32, conflict-free at pitch 17), and splits the 8 pixels of its channel
//     into the three bf16 fragments in registers -- no operand buffer, no extra barrier;
//   * per column a wave runs 2 K-steps of its own tap (2 x 24 MFMAs) and one (K-step, o-tile) piece of tap 8 (6 MFMAs): wave v takes
//     K-step v / 4, o-tile v % 4; the two shares of an o-tile are added through LDS at the end, in wave order.
// One accumulator per (tap, o-tile): a workgroup sums ~900 K-steps, i.e. ~5 400 roundings at the magnitude of the running sum
// against the fp32 kernel's ~14 000 (one per pixel); measured against float64 in tests/test_gpu_split.py.
constexpr int BS_GP = 20;                      // dwords per gy row: 16 (32 bf16) + 4 of padding
constexpr int BS_GYB = 3 * 128 * BS_GP;        // dwords of the gy column buffer (3 pieces)
constexpr int BS_SCRP = 17;                    // scratch row pitch (floats)
constexpr int BS_SCR = 32 * BS_SCRP;           // floats of one wave's transposition scratch
constexpr int BS_X2 = ((2 * BW_XW + 3) / 4) * 4;  // both x windows, rounded so that the gy buffer behind them is 16-byte aligned
constexpr int BS_LDS_DWORDS = BS_X2 + BS_GYB + 8 * BS_SCR;

// the 24 (F16: 12) MFMAs of one K-step of a wave's tap: smallest terms first, consecutive MFMAs on different accumulators
template <bool F16>
__device__ __forceinline__ void bww_mma24(f32x16 (&acc)[4], const uint4 (&a)[4][3], const uint4 (&bf)[3]) {
  if constexpr (F16) {
#define MODE_BS_TERM(PA, PB) _Pragma("unroll") for (int m = 0; m < 4; ++m) acc[m] = mfma_f16(a[m][PA], bf[PB], acc[m]);
    MODE_BS_TERM(1, 0)
    MODE_BS_TERM(0, 1)
    MODE_BS_TERM(0, 0)
#undef MODE_BS_TERM
  } else {
#define MODE_BS_TERM(PA, PB) _Pragma("unroll") for (int m = 0; m < 4; ++m) acc[m] = mfma_bf16(a[m][PA], bf[PB], acc[m]);
    MODE_BS_TERM(2, 0)
    MODE_BS_TERM(0, 2)
    MODE_BS_TERM(1, 1)
    MODE_BS_TERM(1, 0)
    MODE_BS_TERM(0, 1)
    MODE_BS_TERM(0, 0)
#undef MODE_BS_TERM
  }
}

// F16: the two-piece fp16 arithmetic of the other two spherical kernels (3v): gy is scaled by its tensor's power of two when a column is
// committed, the sampled operand through its four bilinear weights, the partial sums by the inverse of both; 12 MFMAs per K-step.
template <bool F16>
__global__ __launch_bounds__(NTHREADS) void sphere_bww_split_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                                     float* __restrict__ part, WinDims d, const int4* __restrict__ tiles,
                                                                     const float4* __restrict__ rec_w, const int* __restrict__ rec_off,
                                                                     int ntiles, int S, const float* __restrict__ amax_g,
                                                                     const float* __restrict__ amax_x) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float sg = 1.f, sx = 1.f, unscale = 1.f;
  if (F16) {
    sg = f16_scale_of(mode::absmax_load(amax_g));
    sx = f16_scale_of(mode::absmax_load(amax_x));
    unscale = (1.f / sg) * (1.f / sx);
  }
  constexpr int NPC = Arith<F16>::NP;  // pieces per value
  uint32_t* gyb = reinterpret_cast<uint32_t*>(smem + BS_X2);  // [3][128][BS_GP]
  constexpr int WRP = BW_WR, CP = BW_CP;
  const int s = blockIdx.x, cg = blockIdx.y;
  const int g = blockIdx.z / d.MG, mg = blockIdx.z % d.MG;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int j = lane & 31, half = lane >> 5;
  float* scr = smem + BS_X2 + BS_GYB + wave * BS_SCR;  // this wave's transposition scratch [32 c][BS_SCRP]
  const long long HW = (long long)d.H * d.W;
  const int T = ntiles * 2 * d.B;  // (sample, tile, half) items
  const int NCG = gridDim.y;

  f32x16 acc[4], acc8;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    acc[0][r] = acc[1][r] = acc[2][r] = acc[3][r] = 0.f;
    acc8[r] = 0.f;
  }
  for (int i = tid; i < BS_LDS_DWORDS; i += NTHREADS) smem[i] = 0.f;  // every word that may be read is finite

  const int omax = d.Cog - mg * 128;
  const int cmax = d.Cig - cg * BW_CG;
  // sampling role of this lane: pixel 16 ks + 8 sh + sp8 of the column, channels 8 sq .. 8 sq + 7 of the chunk
  const int sh = half, sq = j >> 3, sp8 = j & 7;
  const int ks8 = wave >> 2, m8 = wave & 3;  // this wave's piece of tap 8

  struct Item {
    int b, ti, hf, h0, w0, rbase, cbase;
  };
  auto item_of = [&](int t) {
    Item it;
    it.b = t / (ntiles * 2);
    const int r = t - it.b * ntiles * 2;
    it.ti = r >> 1;
    it.hf = r & 1;
    const int4 tl = tiles[it.ti];
    it.h0 = tl.x + it.hf * BW_TH;
    it.w0 = tl.y;
    it.rbase = (tl.z + it.hf * BW_TH) % d.H;
    it.cbase = tl.w & 0xffff;
    return it;
  };
  // x window staging exactly as in sphere_bww_win_kernel
  // (staging coordinates recomputed from an opaque copy of the thread index where they are used -- see issue_gy)
  float pxw[BW_NXW];
  bool pxw_ok = false;
  auto issue_xw = [&](const Item& it, int part) {
    int t_ = tid;
    asm volatile("" : "+v"(t_));
    const int xcol = d.sh == 1 ? t_ >> 6 : t_ & (WC - 1), xrow = d.sh == 1 ? t_ & 63 : t_ >> 3;
    const bool xrow_ok = xrow < WRP;
    pxw_ok = xrow_ok && it.cbase + xcol < d.W;
    const int grow = (it.rbase + (xrow_ok ? xrow : 0)) % d.H;
    const float* xg = x + ((long long)it.b * d.Ci + (long long)g * d.Cig + (long long)cg * BW_CG) * HW +
                      (pxw_ok ? (long long)grow * d.sh + (long long)(it.cbase + xcol) * d.sw : 0);
#pragma unroll
    for (int c = 0; c < BW_NXW; ++c) pxw[c] = xg[(long long)min(part * BW_NXW + c, cmax - 1) * HW];
  };
  auto commit_xw = [&](float* xwdst, int part) {
    int t_ = tid;
    asm volatile("" : "+v"(t_));
    const int xcol = d.sh == 1 ? t_ >> 6 : t_ & (WC - 1), xrow = d.sh == 1 ? t_ & 63 : t_ >> 3;
    if (xrow < WRP) {
      float* dst = xwdst + xcol * WRP + xrow;
#pragma unroll
      for (int c = 0; c < BW_NXW; ++c) dst[(part * BW_NXW + c) * BW_CP] = (pxw_ok && part * BW_NXW + c < cmax) ? pxw[c] : 0.f;
    }
  };
  // gy is requested TWO columns ahead (a column lasts ~1.5 us, less than a trip to HBM under load: with one column of lead the
  // commit between the two barriers waited for it -- measured 0.08 ms of a 0.36 ms call), into two register sets
  const int gpp_ = tid & 15, go0_ = tid >> 4;
  const int gpp = gpp_, go0 = go0_;
  struct GyPF {
    float g0[4], g1[4];
    unsigned ok;  // bit 2u: first pixel of pair real, bit 2u + 1: second
  };
  GyPF gpf[2];
  // records of the next column: own tap at K-steps 0 / 1, tap 8 at K-step ks8 -- for the pixel this lane samples
  float4 prw0, prw1, prw8;
  int pro0, pro1, pro8;
  auto issue_gy = [&](const Item& it, int wc, GyPF& pf) {
    // (gpp / go0 through an opaque copy: the row and the four clamped channel offsets derived from them are loop invariants, and kept
    // across the column loop they were the registers the allocator spilled -- every column began with two scratch reloads, each behind an
    // s_waitcnt vmcnt(0) that also drained the gy requested for the column after next.  Recomputed here they cost ~12 instructions.)
    int gpp = gpp_, go0 = go0_;
    asm volatile("" : "+v"(gpp), "+v"(go0));
    const int h = it.h0 + 2 * gpp, w = it.w0 + wc;
    const bool ok0 = h < d.H && w < d.W, ok1 = h + 1 < d.H && w < d.W;
    const float* gyb0 = gy + ((long long)it.b * d.Co + (long long)g * d.Cog + (long long)mg * 128) * HW +
                        (ok0 ? (long long)h * d.sh + (long long)w * d.sw : 0);
    const long long step1 = ok1 ? d.sh : 0;
    pf.ok = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int o = go0 + 32 * u;
      const float* p = gyb0 + (long long)min(o, omax - 1) * HW;
      pf.g0[u] = p[0];
      pf.g1[u] = p[step1];
      pf.ok |= ((ok0 && o < omax) ? 1u : 0u) << (2 * u) | ((ok1 && o < omax) ? 2u : 0u) << (2 * u);
    }
  };
  auto issue_rec = [&](const Item& it, int wc) {  // records: L2-resident, one column of lead is plenty
    const long long rcol = (((long long)it.ti * 2 + it.hf) * TW + wc) * BW_NREC;
    const int px0 = 8 * sh + sp8;
    prw0 = rec_w[rcol + wave * BW_TH + px0];
    pro0 = rec_off[rcol + wave * BW_TH + px0];
    prw1 = rec_w[rcol + wave * BW_TH + 16 + px0];
    pro1 = rec_off[rcol + wave * BW_TH + 16 + px0];
    prw8 = rec_w[rcol + 8 * BW_TH + 16 * ks8 + px0];
    pro8 = rec_off[rcol + 8 * BW_TH + 16 * ks8 + px0];
  };
  auto commit_col = [&](const GyPF& pf) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float a = (pf.ok >> (2 * u) & 1u) ? pf.g0[u] : 0.f, b2 = (pf.ok >> (2 * u + 1) & 1u) ? pf.g1[u] : 0.f;
      uint32_t p1, p2, p3;
      uint32_t* dst = gyb + (go0 + 32 * u) * BS_GP + gpp;
      if constexpr (F16) {
        split2_f16_mix(a * sg, b2 * sg, p1, p2);
      } else {
        split3_bf16_pinned(a, b2, p1, p2, p3);
        dst[2 * 128 * BS_GP] = p3;
      }
      dst[0] = p1;
      dst[128 * BS_GP] = p2;
    }
  };
  // B fragment of one K-step: sample this lane's pixel for 8 channels, transpose through the scratch, split this lane's channel.
  // No wait between the scratch stores and loads: the LDS serves the instructions of one wave in order, and the compiler keeps
  // may-aliasing LDS accesses in program order -- an explicit s_waitcnt here would pin the whole sample in front of the MFMAs.
  auto sample = [&](const float* xw, const float4 w4_, const int ro, uint4 (&bf)[3]) {
    const float* xb = xw + (8 * sq) * CP + ro;
    float v[8], r_[8][4];
    // (all 32 window words requested before the first is used: as one loop the compiler issued every read right in front of its
    // use -- 16 serialised LDS round trips per sample, three samples per column; see sphere_fwd_split_kernel::sample_read)
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float* q = xb + c * CP;
      r_[c][0] = q[0];
      r_[c][1] = q[WRP];
      r_[c][2] = q[1];
      r_[c][3] = q[WRP + 1];
    }
    __builtin_amdgcn_sched_barrier(0);
    // (F16: the operand's power-of-two scale rides on the four weights)
    const float4 w4 = F16 ? make_float4(w4_.x * sx, w4_.y * sx, w4_.z * sx, w4_.w * sx) : w4_;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      v[c] = __builtin_fmaf(w4.w, r_[c][3], __builtin_fmaf(w4.z, r_[c][2], __builtin_fmaf(w4.y, r_[c][1], w4.x * r_[c][0])));
      asm("" : "+v"(v[c]));
    }
    float* sw = scr + (8 * sq) * BS_SCRP + 8 * sh + sp8;
#pragma unroll
    for (int c = 0; c < 8; ++c) sw[c * BS_SCRP] = v[c];
    const float* sr = scr + j * BS_SCRP + 8 * half;
    float t8[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) t8[i] = sr[i];
    uint32_t q1[4], q2[4], q3[4];
    if constexpr (F16) {
#pragma unroll
      for (int i = 0; i < 4; ++i) split2_f16_mix(t8[2 * i], t8[2 * i + 1], q1[i], q2[i]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) split3_bf16_pinned(t8[2 * i], t8[2 * i + 1], q1[i], q2[i], q3[i]);
      bf[2] = make_uint4(q3[0], q3[1], q3[2], q3[3]);
    }
    bf[0] = make_uint4(q1[0], q1[1], q1[2], q1[3]);
    bf[1] = make_uint4(q2[0], q2[1], q2[2], q2[3]);
  };
  // A fragments (gy, lane = o, 8 consecutive pixels) of the four o-tiles for K-step ks
  auto load_a = [&](int ks, uint4 (&a)[4][3]) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const uint4* ga = reinterpret_cast<const uint4*>(gyb + (m * 32 + j) * BS_GP + 8 * ks + 4 * half);
#pragma unroll
      for (int p = 0; p < NPC; ++p) a[m][p] = ga[p * (128 * BS_GP / 4)];
    }
  };
  auto mma24 = [&](const uint4 (&a)[4][3], const uint4 (&bf)[3]) { bww_mma24<F16>(acc, a, bf); };
  // one MFMA, then up to 4 (F16: 7) vector-ALU instructions and 3 (F16: 4) LDS instructions, n times: spreads a sample (and the next
  // fragment reads) over the matrix instructions issued beside it -- half the MFMAs carry a sample that is three quarters of the work
#define MODE_BS_SPREAD(n)                                            \
  _Pragma("unroll") for (int i_ = 0; i_ < (F16 ? (n) / 2 : (n)); ++i_) { \
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);               \
    __builtin_amdgcn_sched_group_barrier(0x002, F16 ? 7 : 4, 0);     \
    __builtin_amdgcn_sched_group_barrier(0x100, F16 ? 4 : 3, 0);     \
  }                                                                  \
  __builtin_amdgcn_sched_barrier(0);

  Item cur = item_of(s);
  __syncthreads();  // zero fill done
  for (int part = 0; part < TW; ++part) {
    issue_xw(cur, part);
    commit_xw(smem, part);
  }
  issue_gy(cur, 0, gpf[0]);
  issue_rec(cur, 0);
  commit_col(gpf[0]);
  issue_gy(cur, 1, gpf[1]);
  __syncthreads();

  int xbuf = 0;
  uint4 b0[3];
  sample(smem, prw0, pro0, b0);  // K-step 0 of the first column
  for (int t = s; t < T; t += S) {
    const bool more_items = t + S < T;
    const Item nxt = item_of(more_items ? t + S : t);
    const float* xw = smem + xbuf * BW_XW;
#pragma unroll
    for (int wc = 0; wc < TW; ++wc) {  // (unrolled: the gy register set of a column is wc % 2)
      const bool last_col = wc == TW - 1;
      const bool have_next = !last_col || more_items;
      const float4 rw1 = prw1, rw8 = prw8;
      const int ro1 = pro1, ro8 = pro8;
      // Requests in the order they are consumed (vmcnt retires in order): the next item's window part (committed at the end of this
      // column), the next column's records, and last the gy of the column after next (its register set held this column's gy, committed
      // at the end of the previous column) -- requested first, the window commit's wait drained it too.  All unconditional (`nxt` is
      // the current item again when there is no next one): a request under a branch turns the waits behind it into vmcnt(0).
      issue_xw(nxt, wc);
      issue_rec(last_col ? nxt : cur, last_col ? 0 : wc + 1);
      issue_gy(wc < 2 ? cur : nxt, wc < 2 ? wc + 2 : wc - 2, gpf[wc & 1]);
      __builtin_amdgcn_sched_barrier(0);

      uint4 a[4][3], b1[3], b8[3];
      // K-step 0 of the own tap beside the sampling of K-step 1
      load_a(0, a);
      sample(xw, rw1, ro1, b1);
      mma24(a, b0);
      MODE_BS_SPREAD(24)
      // K-step 1 beside the sampling of this wave's piece of tap 8
      load_a(1, a);
      sample(xw, rw8, ro8, b8);
      mma24(a, b1);
      MODE_BS_SPREAD(24)
      // tap 8: o-tile m8, K-step ks8
      {
        const uint4* ga = reinterpret_cast<const uint4*>(gyb + (m8 * 32 + j) * BS_GP + 8 * ks8 + 4 * half);
        const uint4 a1 = ga[0], a2 = ga[128 * BS_GP / 4];
        if constexpr (F16) {
          acc8 = mfma_f16(a2, b8[0], acc8);
          acc8 = mfma_f16(a1, b8[1], acc8);
          acc8 = mfma_f16(a1, b8[0], acc8);
        } else {
          const uint4 a3 = ga[2 * (128 * BS_GP / 4)];
          acc8 = mfma_bf16(a3, b8[0], acc8);
          acc8 = mfma_bf16(a1, b8[2], acc8);
          acc8 = mfma_bf16(a2, b8[1], acc8);
          acc8 = mfma_bf16(a2, b8[0], acc8);
          acc8 = mfma_bf16(a1, b8[1], acc8);
          acc8 = mfma_bf16(a1, b8[0], acc8);
        }
      }
      if (more_items) commit_xw(smem + (xbuf ^ 1) * BW_XW, wc);  // the other window buffer: nobody reads it now

      __syncthreads();  // everyone is done with this column's gy
      if (have_next) commit_col(gpf[(wc + 1) & 1]);
      __syncthreads();
      // K-step 0 of the next column (after the barrier: at an item boundary its window was completed by the commit above)
      if (have_next) sample(last_col ? smem + (xbuf ^ 1) * BW_XW : xw, prw0, pro0, b0);
    }
    cur = nxt;
    xbuf ^= 1;
  }
#undef MODE_BS_SPREAD

  // partials: [tap][128 o][32 c] per (slice, z, channel group), the layout reduce_gw_win sums
  float* pb = part + ((((long long)s * gridDim.z + blockIdx.z) * NCG + cg) * BW_SLOTS) * (128 * BW_CG);
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int o = MODE_ACC_ROW(m, r, half);
      pb[((long long)wave * 128 + o) * BW_CG + j] = F16 ? acc[m][r] * unscale : acc[m][r];
    }
  // tap 8: o-tile m8 = the share of K-step 0 (waves 0..3) + the share of K-step 1 (waves 4..7), added in that order through LDS
  float* red = smem;  // [128 o][32 c]; the item loop ended with a barrier
  if (wave < 4) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[(MODE_ACC_ROW(m8, r, half)) * BW_CG + j] = F16 ? acc8[r] * unscale : acc8[r];
  }
  __syncthreads();
  if (wave >= 4) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[(MODE_ACC_ROW(m8, r, half)) * BW_CG + j] += F16 ? acc8[r] * unscale : acc8[r];
  }
  __syncthreads();
  for (int i = tid; i < 128 * BW_CG; i += NTHREADS) pb[(long long)8 * 128 * BW_CG + i] = red[i];
}

// The same contraction for the polar items (sphere_bww_polar_kernel's work items: one column of 32 pixels with nine per-tap windows,
// staged in place per item), on the split-bf16 arithmetic: the sampling / transposition / MFMA sequence of sphere_bww_split_kernel on
// the per-tap window layout.
constexpr int BQ_X = ((BP_XW + 3) / 4) * 4;
constexpr int BQ_LDS_DWORDS = BQ_X + BS_GYB + 8 * BS_SCR;

__global__ __launch_bounds__(NTHREADS) void sphere_bww_polar_split_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                                           float* __restrict__ part, WinDims d,
                                                                           const int* __restrict__ pitems, const float4* __restrict__ rec_w,
                                                                           const int* __restrict__ rec_off, int nitems, int S, int s_base) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* xw = smem;
  uint32_t* gyb = reinterpret_cast<uint32_t*>(smem + BQ_X);
  constexpr int WRP = BP_WR, CP = BP_CP;
  const int s = blockIdx.x, cg = blockIdx.y;
  const int g = blockIdx.z / d.MG, mg = blockIdx.z % d.MG;
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int j = lane & 31, half = lane >> 5;
  float* scr = smem + BQ_X + BS_GYB + wave * BS_SCR;
  const long long HW = (long long)d.H * d.W;
  const int T = nitems * d.B;
  const int omax = d.Cog - mg * 128, cmax = d.Cig - cg * BW_CG;
  const int sh = half, sq = j >> 3, sp8 = j & 7;
  const int ks8 = wave >> 2, m8 = wave & 3;
  const int gpp = tid & 15, go0 = tid >> 4;

  f32x16 acc[4], acc8;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    acc[0][r] = acc[1][r] = acc[2][r] = acc[3][r] = 0.f;
    acc8[r] = 0.f;
  }
  for (int i = tid; i < BQ_LDS_DWORDS; i += NTHREADS) smem[i] = 0.f;

  constexpr int NE = KT * BP_TAPW;  // 612 window words per channel
  const int e0 = tid, e1 = tid + NTHREADS;
  const bool has1 = e1 < NE;
  const int k0 = e0 / BP_TAPW, k1 = (has1 ? e1 : 0) / BP_TAPW;
  const int col0 = (e0 % BP_TAPW) / BP_WR, r0 = e0 % BP_WR;
  const int col1 = ((has1 ? e1 : 0) % BP_TAPW) / BP_WR, r1 = (has1 ? e1 : 0) % BP_WR;

  auto sample = [&](const float4 w4, const int ro, uint4 (&bf)[3]) {
    const float* xb = xw + (8 * sq) * CP + ro;
    float v[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float* q = xb + c * CP;
      v[c] = __builtin_fmaf(w4.w, q[WRP + 1], __builtin_fmaf(w4.z, q[1], __builtin_fmaf(w4.y, q[WRP], w4.x * q[0])));
      asm("" : "+v"(v[c]));
    }
    float* sw = scr + (8 * sq) * BS_SCRP + 8 * sh + sp8;
#pragma unroll
    for (int c = 0; c < 8; ++c) sw[c * BS_SCRP] = v[c];
    const float* sr = scr + j * BS_SCRP + 8 * half;
    float t8[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) t8[i] = sr[i];
    uint32_t q1[4], q2[4], q3[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) split3_bf16_pinned(t8[2 * i], t8[2 * i + 1], q1[i], q2[i], q3[i]);
    bf[0] = make_uint4(q1[0], q1[1], q1[2], q1[3]);
    bf[1] = make_uint4(q2[0], q2[1], q2[2], q2[3]);
    bf[2] = make_uint4(q3[0], q3[1], q3[2], q3[3]);
  };
  auto load_a = [&](int ks, uint4 (&a)[4][3]) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const uint4* ga = reinterpret_cast<const uint4*>(gyb + (m * 32 + j) * BS_GP + 8 * ks + 4 * half);
#pragma unroll
      for (int p = 0; p < 3; ++p) a[m][p] = ga[p * (128 * BS_GP / 4)];
    }
  };
  auto mma24 = [&](const uint4 (&a)[4][3], const uint4 (&bf)[3]) { bww_mma24<false>(acc, a, bf); };

  // Staging of an item without serial round trips (it used to be: the item's table words, then four `#pragma unroll 1` rounds of
  // 16 x loads -> LDS stores, then the gy loads -> stores, then the tap records -- six or seven exposed memory latencies in front of
  // about 1 us of MFMAs, with one workgroup per CU and nothing else to hide them).  Now every global load of the item (64 x words, 8 gy
  // words, the 3 tap records) is issued in one batch into registers BEFORE the barrier that waits for the previous item's consumers --
  // a wave that is done with item t has the loads of the next item in flight while the others finish -- and committed to LDS after it;
  // the table words of the item after that are requested behind the batch and are there a whole item later.  (No room for a second
  // window buffer in LDS.  Keeping the batch of item t + S in registers across the sample / MFMA phase of item t was built too -- it fits
  // in 256 registers once the phase holds the gy fragments of two row blocks at a time -- and measured the same 62.6 us per launch:
  // with the round trips gone the loads are no longer what an item waits for, so the simpler form stayed.)  What lands in LDS, and
  // everything from there on, is unchanged.
  auto item_words = [&](int t, int (&pv)[6]) {
    const int* pi = pitems + (long long)(t % nitems) * BP_ITEM_INTS;
    pv[0] = pi[0]; pv[1] = pi[1];
    pv[2] = pi[2 + k0]; pv[3] = pi[2 + KT + k0]; pv[4] = pi[2 + k1]; pv[5] = pi[2 + KT + k1];
  };
  int pv[6] = {0, 0, 0, 0, 0, 0};
  if (s < T) item_words(s, pv);
  for (int t = s; t < T; t += S) {
    const int b = t / nitems, it = t - b * nitems;
    const int h0 = pv[0], w = pv[1];
    const int rb0 = pv[2], cb0 = pv[3], rb1 = pv[4], cb1 = pv[5];
    const bool xok0 = cb0 + col0 < d.W, xok1 = has1 && cb1 + col1 < d.W;
    // (opaque copies: the 32 + 4 lane masks of the channel bounds are loop invariants, and hoisted they cost 70 scalar registers)
    int cmx = cmax, omx = omax;
    asm volatile("" : "+s"(cmx), "+s"(omx));
    float xv0[BW_CG], xv1[BW_CG];
    {
      const float* xg = x + ((long long)b * d.Ci + (long long)g * d.Cig + (long long)cg * BW_CG) * HW;
      const long long a0 = xok0 ? (long long)((rb0 + r0) % d.H) * d.sh + (long long)(cb0 + col0) * d.sw : 0;
      const long long a1 = xok1 ? (long long)((rb1 + r1) % d.H) * d.sh + (long long)(cb1 + col1) * d.sw : 0;
      const float* xc = xg;  // channel min(c, cmax - 1), stepped (32 hoisted 64-bit plane offsets do not fit the scalar registers)
#pragma unroll
      for (int c = 0; c < BW_CG; ++c) {
        xv0[c] = xc[a0];
        xv1[c] = xc[a1];
        if (c + 1 < cmx) xc += HW;
      }
    }
    const int gh = h0 + 2 * gpp;
    const bool gok0 = gh < d.H && w < d.W, gok1 = gh + 1 < d.H && w < d.W;
    float gv0[4], gv1[4];
    {
      const float* gyb0 = gy + ((long long)b * d.Co + (long long)g * d.Cog + (long long)mg * 128) * HW +
                          (gok0 ? (long long)gh * d.sh + (long long)w * d.sw : 0);
      const long long step1 = gok1 ? d.sh : 0;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float* p = gyb0 + (long long)min(go0 + 32 * u, omx - 1) * HW;
        gv0[u] = p[0];
        gv1[u] = p[step1];
      }
    }
    const long long rbase = (long long)it * BW_NREC;
    const int px0 = 8 * sh + sp8;
    const float4 rw0 = rec_w[rbase + wave * BW_TH + px0], rw1 = rec_w[rbase + wave * BW_TH + 16 + px0];
    const float4 rw8 = rec_w[rbase + 8 * BW_TH + 16 * ks8 + px0];
    const int ro0 = rec_off[rbase + wave * BW_TH + px0], ro1 = rec_off[rbase + wave * BW_TH + 16 + px0];
    const int ro8 = rec_off[rbase + 8 * BW_TH + 16 * ks8 + px0];
    if (t + S < T) item_words(t + S, pv);  // (read at the top of the next pass)
    __syncthreads();  // previous item consumed (first pass: zero fill done)
#pragma unroll
    for (int c = 0; c < BW_CG; ++c) {
      xw[c * BP_CP + e0] = (xok0 && c < cmx) ? xv0[c] : 0.f;
      if (has1) xw[c * BP_CP + e1] = (xok1 && c < cmx) ? xv1[c] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool oo = go0 + 32 * u < omx;
      uint32_t p1, p2, p3;
      split3_bf16_pinned((gok0 && oo) ? gv0[u] : 0.f, (gok1 && oo) ? gv1[u] : 0.f, p1, p2, p3);
      uint32_t* dst = gyb + (go0 + 32 * u) * BS_GP + gpp;
      dst[0] = p1;
      dst[128 * BS_GP] = p2;
      dst[2 * 128 * BS_GP] = p3;
    }
    __syncthreads();
    uint4 a[4][3], b0[3], b1[3], b8[3];
    sample(rw0, ro0, b0);
    load_a(0, a);
    sample(rw1, ro1, b1);
    mma24(a, b0);
    load_a(1, a);
    sample(rw8, ro8, b8);
    mma24(a, b1);
    {
      const uint4* ga = reinterpret_cast<const uint4*>(gyb + (m8 * 32 + j) * BS_GP + 8 * ks8 + 4 * half);
      const uint4 a1 = ga[0], a2 = ga[128 * BS_GP / 4], a3 = ga[2 * (128 * BS_GP / 4)];
      acc8 = mfma_bf16(a3, b8[0], acc8);
      acc8 = mfma_bf16(a1, b8[2], acc8);
      acc8 = mfma_bf16(a2, b8[1], acc8);
      acc8 = mfma_bf16(a2, b8[0], acc8);
      acc8 = mfma_bf16(a1, b8[1], acc8);
      acc8 = mfma_bf16(a1, b8[0], acc8);
    }
  }
  __syncthreads();
  float* pb = part + ((((long long)(s_base + s) * gridDim.z + blockIdx.z) * gridDim.y + cg) * BW_SLOTS) * (128 * BW_CG);
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int o = MODE_ACC_ROW(m, r, half);
      pb[((long long)wave * 128 + o) * BW_CG + j] = acc[m][r];
    }
  float* red = smem;
  if (wave < 4) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[(MODE_ACC_ROW(m8, r, half)) * BW_CG + j] = acc8[r];
  }
  __syncthreads();
  if (wave >= 4) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[(MODE_ACC_ROW(m8, r, half)) * BW_CG + j] += acc8[r];
  }
  __syncthreads();
  for (int i = tid; i < 128 * BW_CG; i += NTHREADS) pb[(long long)8 * 128 * BW_CG + i] = red[i];
}

}  // namespace

int bww_polar_splits(const WinDims& d, int n_items) {
  const int T = n_items * d.B;
  const int wgs_per_slice = mode::cdiv(d.Cig, BW_CG) * d.G * d.MG;
  const int per = std::max(1, mode::cdiv((long long)T * wgs_per_slice, kNumCU));
  return std::max(1, mode::cdiv(T, per));
}

extern "C" size_t mode_sphere_conv_bwd_weight_win_workspace_bytes(int B, int Ci, int H, int W, int Co, int Kh, int Kw, int groups,
                                                                  int n_small, int n_rest_pixels, int n_polar_items) {
  WinDims d;
  if (make_win_dims(d, B, Ci, H, W, Co, Kh, Kw, groups, "mode_sphere_conv_bwd_weight_win_workspace_bytes") != MODE_OK) return 0;
  const size_t slice = (size_t)d.G * d.MG * mode::cdiv(d.Cig, BW_CG) * BW_SLOTS * 128 * BW_CG * sizeof(float);
  const size_t win = slice * (bww_win_splits(d, std::max(n_small, 1)) + bww_polar_splits(d, std::max(n_polar_items, 1)));
  return win + mode::sphere_bwd_weight_general_workspace(B, Ci, Co, Kh, Kw, H, W, groups, std::max(n_rest_pixels, 1));
}

// Weight gradient, ADDED to gw like mode_sphere_conv_bwd_weight: windowed kernel on the n_small compact tiles of the plan
// (tile list order: wrap-around, mid, small), the polar kernel on the n_polar_items column items of the other tiles
// (mode_sphere_plan_polar), or -- when those could not be planned -- the general kernels on their n_rest_pixels pixels.
static int bwd_weight_win_impl(const float* gy, const float* pos, const float* x, float* gw, float* workspace, const int32_t* tiles,
                               int n_small, int n_mid, int n_wrap, const float* rec_w, const int32_t* rec_off, const int32_t* rest_pixels,
                               int n_rest_pixels, const int32_t* pitems, const float* prec_w, const int32_t* prec_off, int n_polar_items,
                               int B, int Ci, int H, int W, int Co, int Kh, int Kw, int groups, const float* gy_t, const float* x_t,
                               mode_stream_t stream, int split, const float* amax_g = nullptr, const float* amax_x = nullptr);

extern "C" int mode_sphere_conv_bwd_weight_win(const float* gy, const float* pos, const float* x, float* gw, float* workspace,
                                               const int32_t* tiles, int n_small, int n_mid, int n_wrap, const float* rec_w,
                                               const int32_t* rec_off, const int32_t* rest_pixels, int n_rest_pixels,
                                               const int32_t* pitems, const float* prec_w, const int32_t* prec_off, int n_polar_items,
                                               int B, int Ci, int H, int W, int Co, int Kh, int Kw, int groups, const float* gy_t,
                                               const float* x_t, mode_stream_t stream) {
  return bwd_weight_win_impl(gy, pos, x, gw, workspace, tiles, n_small, n_mid, n_wrap, rec_w, rec_off, rest_pixels, n_rest_pixels, pitems,
                             prec_w, prec_off, n_polar_items, B, Ci, H, W, Co, Kh, Kw, groups, gy_t, x_t, stream, 0);
}

// The same with the compact-window tiles on the split-bf16 kernel (sphere_bww_split_kernel: fp32 operands split exactly into three
// bf16 pieces, six bf16 MFMAs per product, fp32 accumulation); polar items and listed pixels as above.
extern "C" int mode_sphere_conv_bwd_weight_win_split(const float* gy, const float* pos, const float* x, float* gw, float* workspace,
                                                     const int32_t* tiles, int n_small, int n_mid, int n_wrap, const float* rec_w,
                                                     const int32_t* rec_off, const int32_t* rest_pixels, int n_rest_pixels,
                                                     const int32_t* pitems, const float* prec_w, const int32_t* prec_off,
                                                     int n_polar_items, int B, int Ci, int H, int W, int Co, int Kh, int Kw, int groups,
                                                     const float* gy_t, const float* x_t, mode_stream_t stream) {
  return bwd_weight_win_impl(gy, pos, x, gw, workspace, tiles, n_small, n_mid, n_wrap, rec_w, rec_off, rest_pixels, n_rest_pixels, pitems,
                             prec_w, prec_off, n_polar_items, B, Ci, H, W, Co, Kh, Kw, groups, gy_t, x_t, stream, 1);
}

// The split call with the compact-window tiles on the two-piece fp16 arithmetic (3v): amax_g / amax_x = the maximum buffers of gy and x
// (the polar items keep three bf16 pieces; their partial sums go through the same reduction).
extern "C" int mode_sphere_conv_bwd_weight_win_split_f16(const float* gy, const float* pos, const float* x, const float* amax_g,
                                                         const float* amax_x, float* gw, float* workspace, const int32_t* tiles, int n_small,
                                                         int n_mid, int n_wrap, const float* rec_w, const int32_t* rec_off,
                                                         const int32_t* rest_pixels, int n_rest_pixels, const int32_t* pitems,
                                                         const float* prec_w, const int32_t* prec_off, int n_polar_items, int B, int Ci, int H,
                                                         int W, int Co, int Kh, int Kw, int groups, const float* gy_t, const float* x_t,
                                                         mode_stream_t stream) {
  MODE_REQUIRE(amax_g && amax_x, MODE_ERR_BAD_ARG, "mode_sphere_conv_bwd_weight_win_split_f16: null maximum");
  return bwd_weight_win_impl(gy, pos, x, gw, workspace, tiles, n_small, n_mid, n_wrap, rec_w, rec_off, rest_pixels, n_rest_pixels, pitems,
                             prec_w, prec_off, n_polar_items, B, Ci, H, W, Co, Kh, Kw, groups, gy_t, x_t, stream, 1, amax_g, amax_x);
}

static int bwd_weight_win_impl(const float* gy, const float* pos, const float* x, float* gw, float* workspace, const int32_t* tiles,
                               int n_small, int n_mid, int n_wrap, const float* rec_w, const int32_t* rec_off, const int32_t* rest_pixels,
                               int n_rest_pixels, const int32_t* pitems, const float* prec_w, const int32_t* prec_off, int n_polar_items,
                               int B, int Ci, int H, int W, int Co, int Kh, int Kw, int groups, const float* gy_t, const float* x_t,
                               mode_stream_t stream, int split, const float* amax_g, const float* amax_x) {
  WinDims d;
  int rc = make_win_dims(d, B, Ci, H, W, Co, Kh, Kw, groups, "mode_sphere_conv_bwd_weight_win");
  MODE_REQUIRE((amax_g == nullptr) == (amax_x == nullptr), MODE_ERR_BAD_ARG, "mode_sphere_conv_bwd_weight_win: both operand maxima, or neither");
  if (rc != MODE_OK) return rc;
  MODE_REQUIRE((gy_t == nullptr) == (x_t == nullptr), MODE_ERR_BAD_ARG, "mode_sphere_conv_bwd_weight_win: gy_t and x_t come together");
  if (gy_t) {
    d.sh = 1;
    d.sw = H;
  }
  MODE_REQUIRE(n_small >= 0 && n_mid >= 0 && n_wrap >= 0 && n_rest_pixels >= 0 && n_polar_items >= 0 &&
                   (size_t)n_small + n_mid + n_wrap == mode_sphere_plan_max_tiles(H, W),
               MODE_ERR_BAD_ARG, "mode_sphere_conv_bwd_weight_win: the plan must cover every tile");
  if (B == 0) return MODE_OK;
  // (the NCHW tensors are only read by the pixel-list fallback: with the transposed copies and no listed pixel they may be null)
  MODE_REQUIRE(((gy && x) || (gy_t && n_rest_pixels == 0)) && pos && gw && workspace && tiles && (n_rest_pixels == 0 || rest_pixels) &&
                   (n_small == 0 || (rec_w && rec_off)) &&
                   (n_polar_items == 0 || (pitems && prec_w && prec_off)),
               MODE_ERR_BAD_ARG, "mode_sphere_conv_bwd_weight_win: null pointer");
  hipStream_t st = mode::as_stream(stream);
  const int NCG = mode::cdiv(d.Cig, BW_CG);
  const size_t slice = (size_t)d.G * d.MG * NCG * BW_SLOTS * 128 * BW_CG * sizeof(float);
  const float* gys = gy_t ? gy_t : gy;
  const float* xs = x_t ? x_t : x;
  int S = 0;
  if (n_small > 0) {
    S = bww_win_splits(d, n_small);
    const dim3 grid(S, NCG, d.G * d.MG);
    const int4* tl = reinterpret_cast<const int4*>(tiles) + n_wrap + n_mid;
    const float4* rw = reinterpret_cast<const float4*>(rec_w);
    if (split)
      rc = launch_win("mode_sphere_conv_bwd_weight_win_split", amax_g ? sphere_bww_split_kernel<true> : sphere_bww_split_kernel<false>, grid,
                      (size_t)BS_LDS_DWORDS * sizeof(float), st, gys, xs, workspace, d, tl, rw, rec_off, n_small, S, amax_g, amax_x);
    else
      rc = launch_win("mode_sphere_conv_bwd_weight_win", sphere_bww_win_kernel, grid, (size_t)BW_LDS_FLOATS * sizeof(float), st, gys, xs,
                      workspace, d, tl, rw, rec_off, n_small, S);
    if (rc != MODE_OK) return rc;
  }
  int Sp = 0;
  if (n_polar_items > 0) {
    Sp = bww_polar_splits(d, n_polar_items);
    rc = launch_win("mode_sphere_conv_bwd_weight_win(polar)", split ? sphere_bww_polar_split_kernel : sphere_bww_polar_kernel,
                    dim3(Sp, NCG, d.G * d.MG), (size_t)(split ? BQ_LDS_DWORDS : BP_LDS_FLOATS) * sizeof(float), st, gys, xs, workspace, d, pitems,
                    reinterpret_cast<const float4*>(prec_w), prec_off, n_polar_items, Sp, S);
    if (rc != MODE_OK) return rc;
  }
  if (S + Sp > 0) {
    const long long n = (long long)d.G * d.MG * NCG * KT * 128 * BW_CG;
    hipLaunchKernelGGL(reduce_gw_win, dim3(mode::cdiv(n, 256)), dim3(256), 0, st, workspace, gw, d, S + Sp, NCG);
    rc = mode::check_launch("mode_sphere_conv_bwd_weight_win(reduce)");
    if (rc != MODE_OK) return rc;
  }
  if (n_rest_pixels > 0)
    return mode::sphere_bwd_weight_general(gy, pos, x, gw, reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + slice * (S + Sp)), B,
                                           Ci, H, W, Co, Kh, Kw, 1, 1, H, W, groups, rest_pixels, n_rest_pixels, st,
                                           "mode_sphere_conv_bwd_weight_win(rest)");
  return MODE_OK;
}
