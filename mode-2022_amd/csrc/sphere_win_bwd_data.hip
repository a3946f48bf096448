// Spherical convolution, "windowed" input-gradient kernel for gfx950 (MI355X).  sphere_win_internal.h says what a window is.
#include "sphere_win_internal.h"

// =====================================================================================================================
// Input gradient on the split-bf16 matrix path: the ADJOINT of the sampling as a windowed gather.
//
//   gx[c][q] = sum_{k, o} W[o][c][k] * G_k[o][q],     G_k[o][q] = sum_{(p, wt) in L(k, q)} wt * gy[o][p]
//
// L(k, q) = the output pixels whose tap k touches input pixel q (the transpose of the sampling table; cu:293-356 scatters the same
// terms with atomics).  Away from the poles the table moves slowly, so L(k, q) has at most four entries and the sources of a 64 x 4
// block of q fall into the same compact window of gy that the forward kernel stages of x.  The host plans every tile from the actual
// table (mode_sphere_adjplan_build): tiles whose lists all have <= 4 entries inside an 81-row x 8-column window get records of
// 4 (window offset, weight) slots per (pixel, tap) and run here -- the structure of sphere_fwd_split_kernel, with the sampling
// record read from the plan instead of computed from the table: gy window of 16 channels in LDS (fp32, double-buffered), every wave
// samples its 32 pixels for the next tap into an LDS operand buffer (exact 3-way bf16 split), one output-channel tile per wave for the
// MFMAs.  All other tiles (next to the poles, and the few columns where a list has 5 or 6 entries) stay on the gather kernel of
// sphere_conv.hip, restricted to a tile list (mode_sphere_conv_bwd_data_adj_list).
namespace {


// NS = 4: every adjoint list of the tile has at most four entries; NS = 6: up to six (the columns around the equator, where the
// sampling positions of neighbouring output columns straddle a pixel boundary): slots 4 and 5 come from a second record array, read
// when the tap is sampled (one tile in sixteen: not worth prefetch registers in a kernel at 249 VGPRs).
// F16: the two-piece fp16 arithmetic of the training forward (sphere_fwd_split_kernel<false, true>): sx = the power-of-two scale of gy
// (on the record's weights when a record becomes current), unscale = 1 / (sx * the weights' scale) on the accumulators.
template <int NS, bool F16>
__device__ __forceinline__ void bwd_data_tile(const float* __restrict__ gy, const uint4* __restrict__ wps, float* __restrict__ gx,
                                              const WinDims& d /* roles swapped: Ci = gy channels */, int NCH16, const int4 t,
                                              const int4* __restrict__ rec_off, const float4* __restrict__ rec_w,
                                              const int2* __restrict__ rec_off2, const float2* __restrict__ rec_w2, float* smem,
                                              float sx, float unscale) {
  constexpr int WRP = WR_SMALL, CP = SP_CP;
  uint4* opbuf = reinterpret_cast<uint4*>(smem + SP_WIN_FLOATS);  // [3][8 pixel groups][3 pieces][64 lanes]
  const int h0 = t.x, w0 = t.y, rbase = t.z, cbase = t.w & 0xffff;
  const int b = blockIdx.y;
  const int g = blockIdx.z / d.MG, mg = blockIdx.z % d.MG;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, half = lane >> 5;
  const long long HW = (long long)d.H * d.W;

  // records of the pixel this lane SAMPLES (column wave % 4, row block wave / 4, row lane & 31), one (int4, float4) per tap
  // (uniform bases + one 32-bit lane index: four per-lane 64-bit pointers were 8 registers the six-source tiles do not have)
  const long long rtile = (long long)blockIdx.x * KT * AJ_PIX;
  const int4* rop = rec_off + rtile;
  const float4* rwp = rec_w + rtile;
  const int2* rop2 = rec_off2 + rtile;
  const float2* rwp2 = rec_w2 + rtile;
  const unsigned rlane = wave * 32 + (lane & 31);
  // records: taps 0 and 1 for the two prologue samples, tap 2 for the first tap of the loop; inside the loop the record of the tap
  // after the next sampled one is requested at the top of a tap (L2-resident, shared by all samples and layers of the geometry)
  auto record = [&](int kk, int4& o4, float4& w4, int2& o2, float2& w2) {
    // (the lane index goes through an opaque asm: otherwise the 9 x 4 per-tap addresses are hoisted out of the tap loop as 64-bit
    // per-lane pointers -- 72 registers, spilled and reloaded with a full vmcnt(0) in front of every record load)
    unsigned l = rlane;
    asm volatile("" : "+v"(l));
    o4 = rop[kk * AJ_PIX + l];
    w4 = rwp[kk * AJ_PIX + l];
    o2 = make_int2(0, 0);
    w2 = make_float2(0.f, 0.f);
    if (NS == 6) {
      o2 = rop2[kk * AJ_PIX + l];
      w2 = rwp2[kk * AJ_PIX + l];
    }
  };
  // (F16) the operand's power-of-two scale rides on the record's weights: sx * (sum of w_i g_i) bit for bit
  auto scaled = [&](float4& w4, float2& w2) {
    if (F16) {
      w4 = make_float4(w4.x * sx, w4.y * sx, w4.z * sx, w4.w * sx);
      if (NS == 6) w2 = make_float2(w2.x * sx, w2.y * sx);
    }
  };
  int4 o_p0, o_p1, o_use, o_next;
  float4 w_p0, w_p1, w_use, w_next;
  int2 o2_p0, o2_p1, o2_use, o2_next;
  float2 w2_p0, w2_p1, w2_use, w2_next;
  record(0, o_p0, w_p0, o2_p0, w2_p0);
  record(1, o_p1, w_p1, o2_p1, w2_p1);
  record(2, o_use, w_use, o2_use, w2_use);
  scaled(w_p0, w2_p0);
  scaled(w_p1, w2_p1);
  scaled(w_use, w2_use);

  // every window word that may be read is finite: the staging stores write all rows and columns of both windows; what they never write
  // is the pad word behind each channel, the slack behind the two buffers, and -- during the first chunk -- the head of the second
  // window, into which the last channel of the first runs over (all read only under zero weights)
  if (tid < 2 * SP_CCH) smem[(tid / SP_CCH) * SP_WIN + (tid % SP_CCH) * CP + WC * WRP] = 0.f;
  if (tid < WRP + 8) smem[SP_WIN + tid] = 0.f;
  for (int i = 2 * SP_WIN + tid; i < SP_WIN_FLOATS; i += NTHREADS) smem[i] = 0.f;
  // (no barrier: see sphere_fwd_split_kernel -- the one behind the first window's stores is enough)

  // window staging exactly as in sphere_fwd_split_kernel
  const int scol = d.sh == 1 ? tid / SROWS : tid & (WC - 1), srow = d.sh == 1 ? tid % SROWS : tid / WC;
  const int gcol = cbase + scol;
  const bool col_ok = gcol < d.W;
  const float* xg = gy + ((long long)b * d.Ci + (long long)g * d.Cig) * HW;
  unsigned rowoff[2];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    const int r = rb * SROWS + srow;
    rowoff[rb] = 4u * (unsigned)(((rbase + (r < WRP ? r : 0)) % d.H) * d.sh + (col_ok ? gcol * d.sw : 0));
  }
  const long long plane_bytes = 4 * HW;
  float lv[8][4];
  auto issue = [&](int ch, int ph, int set) {
    const char* xc = reinterpret_cast<const char*>(xg) + ((long long)ch * SP_CCH + ph * 2) * plane_bytes;
#pragma unroll
    for (int cc = 0; cc < 2; ++cc)
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) lv[set][cc * 2 + rb] = *reinterpret_cast<const float*>(xc + cc * plane_bytes + rowoff[rb]);
  };
  auto commit = [&](int ch, int ph, int set, float* buf) {
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
      const int c = ph * 2 + cc;
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) {
        const int r = rb * SROWS + srow;
        float* dst = r < WRP ? buf + c * CP + scol * WRP + r : smem + 2 * SP_WIN + (tid & 7);
        *dst = col_ok ? lv[set][cc * 2 + rb] : 0.f;
      }
    }
  };
  // B fragment of this lane's pixel for one tap: G_k[o][q] for 8 channels o, <= 4 sources each, split, stored as this wave's group
  auto sample = [&](const float* win, const int4 o4, const float4 tw, const int2 o2, const float2 t2, uint4* op) {
    const float* p = win + half * 8 * CP;
    float v[8], r_[8][NS];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float* q = p + c * CP;
      r_[c][0] = q[o4.x];
      r_[c][1] = q[o4.y];
      r_[c][2] = q[o4.z];
      r_[c][3] = q[o4.w];
      if (NS == 6) {
        r_[c][4] = q[o2.x];
        r_[c][5] = q[o2.y];
      }
    }
    __builtin_amdgcn_sched_barrier(0);  // (all window words requested before the first one is used)
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      v[c] = __builtin_fmaf(tw.w, r_[c][3], __builtin_fmaf(tw.z, r_[c][2], __builtin_fmaf(tw.y, r_[c][1], tw.x * r_[c][0])));
      if (NS == 6) v[c] = __builtin_fmaf(t2.y, r_[c][NS - 1], __builtin_fmaf(t2.x, r_[c][NS - 2], v[c]));
      asm("" : "+v"(v[c]));  // (keeps the chains of two channels from being SLP-packed pairwise, see sphere_fwd_split_kernel)
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

  f32x16 acc[4];
#pragma unroll
  for (int gi = 0; gi < 4; ++gi)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[gi][r] = 0.f;
  const int m = wave % TW, gset = (wave / TW) * 4;
  const uint4* wpa = wps + ((long long)(g * d.MG + mg) * NCH16) * KT * MTW * 192 + m * 192;
  const int nsteps = NCH16 * KT;
  constexpr int NPC = Arith<F16>::NP;  // pieces per value
  uint4 acur[3], anxt[3];  // weight fragments of this tap and of the next one
#pragma unroll
  for (int p = 0; p < NPC; ++p) acur[p] = wpa[(unsigned)(p * 64 + lane)];

#pragma unroll
  for (int ph = 0; ph < 8; ++ph) issue(0, ph, ph);
#pragma unroll
  for (int ph = 0; ph < 8; ++ph) commit(0, ph, ph, smem);
  __syncthreads();
  // ---- the tap loop: the slot schedule of sphere_fwd_split_kernel (three operand buffers, sampling two taps ahead, one fragment set
  // refilled in place, window words in two half batches of 4 channels); here a sample has NS sources at arbitrary window offsets
  sample(smem, o_p0, w_p0, o2_p0, w2_p0, opbuf);
  sample(smem, o_p1, w_p1, o2_p1, w2_p1, opbuf + SP_OP);
  lds_barrier();
  uint4 b0[4], b0n[4], b1[4], b2[4];
  const uint4* fragbase = opbuf + gset * 192 + lane;
#pragma unroll
  for (int gi = 0; gi < 4; ++gi) b0[gi] = fragbase[(gi * 3 + 0) * 64];
  constexpr int LAG = NS == 6 ? 1 : 2;  // (six-source tiles hold 8 more window words and 8 more record words: one tap less of staging in flight)
  float raw[4][NS], v[8], ra[4], rb[4];
  uint32_t q1[4], q2[4], q3[4];
  auto words = [&](const float* win, const int4 o4, const int2 o2, int hb) {
    const float* p = win + half * 8 * CP;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float* q = p + (hb * 4 + c) * CP;
      raw[c][0] = q[o4.x];
      raw[c][1] = q[o4.y];
      raw[c][2] = q[o4.z];
      raw[c][3] = q[o4.w];
      if (NS == 6) {
        raw[c][4] = q[o2.x];
        raw[c][5] = q[o2.y];
      }
    }
  };
  words(smem, o_use, o2_use, 0);
  if constexpr (F16) {
    // ---- 12 slots, as in sphere_fwd_split_kernel<false, true>: hi x hi, lo x hi, hi x lo; the second half batch of window words in
    // registers of its own, requested at the top of the tap.  (The empty asm behind each MFMA pins it to its slot: without a consumer in
    // the slot the compiler sinks the first eight below all their sched_barriers, to where their operands' registers are assembled.)
    float raw2[4][NS];
    // Three record sets, the record of sampled tap s in set s % 3, requested FOUR taps ahead (at the top of tap s - 6 ... i.e. under tap
    // k the record of tap k + 4 is requested and the one of tap k + 3 becomes current in slot 8): requested one tap ahead as in the
    // three-piece loop it would be the newest request when slot 8 needs it -- a vmcnt(0) that also drains the window staging loads
    // of the previous tap, which have two taps to arrive.
    int4 ro[3];
    float4 rwt[3];
    int2 ro2[3];
    float2 rwt2[3];
    ro[2] = o_use; rwt[2] = w_use; ro2[2] = o2_use; rwt2[2] = w2_use;  // (already scaled)
    record(3, ro[0], rwt[0], ro2[0], rwt2[0]);
    for (int ch = 0; ch < NCH16; ++ch) {
      float* cur = smem + (ch & 1) * SP_WIN;
      float* nxt = smem + ((ch + 1) & 1) * SP_WIN;
      const int chn = ch + 1 < NCH16 ? ch + 1 : ch;
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        const int step = ch * KT + k;
        const int nstep = step + 1 < nsteps ? step + 1 : nsteps - 1;
        const float* wsrc = k + 2 < KT ? cur : nxt;
        const float* wsrcn = k + 3 < KT ? cur : nxt;
        const uint4* fcur = fragbase + (k % 3) * SP_OP;
        const uint4* fnxt = fragbase + ((k + 1) % 3) * SP_OP;
        uint4* opw = opbuf + ((k + 2) % 3) * SP_OP + (wave * 3) * 64 + lane;
        const int su = (k + 2) % 3, sn = (k + 3) % 3, sl = (k + 4) % 3;  // sets: current, next, the one being requested
        auto combine = [&](int c, float (&rr)[4][NS]) {
          const float4 tw = rwt[su];
          float t = __builtin_fmaf(tw.w, rr[c & 3][3], __builtin_fmaf(tw.z, rr[c & 3][2], __builtin_fmaf(tw.y, rr[c & 3][1], tw.x * rr[c & 3][0])));
          if (NS == 6) t = __builtin_fmaf(rwt2[su].y, rr[c & 3][NS - 1], __builtin_fmaf(rwt2[su].x, rr[c & 3][NS - 2], t));
          v[c] = t;
          asm("" : "+v"(v[c]));
        };
        auto hsplit = [&](int j) { split2_f16_mix(v[2 * j], v[2 * j + 1], q1[j], q2[j]); };
#pragma unroll
        for (int p = 0; p < 2; ++p) anxt[p] = (wpa + (long long)nstep * MTW * 192)[(unsigned)(p * 64 + lane)];
        record((k + 4) % KT, ro[sl], rwt[sl], ro2[sl], rwt2[sl]);
        {
          const float* p = wsrc + half * 8 * CP;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float* q = p + (4 + c) * CP;
            raw2[c][0] = q[ro[su].x];
            raw2[c][1] = q[ro[su].y];
            raw2[c][2] = q[ro[su].z];
            raw2[c][3] = q[ro[su].w];
            if (NS == 6) {
              raw2[c][4] = q[ro2[su].x];
              raw2[c][5] = q[ro2[su].y];
            }
          }
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
        // the record of the tap sampled under the NEXT tap becomes current; its first half batch of window words is requested here
        scaled(rwt[sn], rwt2[sn]);
#pragma unroll
        for (int gi = 0; gi < 4; ++gi) b0n[gi] = fnxt[(gi * 3 + 0) * 64];
        words(wsrcn, ro[sn], ro2[sn], 0);
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
        if (k >= LAG && k < 4 + LAG) commit(chn, 2 * (k - LAG), 2 * (k - LAG), nxt);
        MODE_SB
        MODE_MFH(0, b1, 3) MODE_SB
        if (k >= LAG && k < 4 + LAG) commit(chn, 2 * (k - LAG) + 1, 2 * (k - LAG) + 1, nxt);
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
    const int chn = ch + 1 < NCH16 ? ch + 1 : ch;
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      const int step = ch * KT + k;
      const int nstep = step + 1 < nsteps ? step + 1 : nsteps - 1;
      const float* wsrc = k + 2 < KT ? cur : nxt;           // window of the tap sampled under this one (tap (k + 2) % 9)
      const float* wsrcn = k + 3 < KT ? cur : nxt;          // ... and of the one sampled under the next tap
      const uint4* fcur = fragbase + (k % 3) * SP_OP;
      const uint4* fnxt = fragbase + ((k + 1) % 3) * SP_OP;
      uint4* opw = opbuf + ((k + 2) % 3) * SP_OP + (wave * 3) * 64 + lane;
      auto combine = [&](int c) {
        float t = __builtin_fmaf(w_use.w, raw[c & 3][3], __builtin_fmaf(w_use.z, raw[c & 3][2], __builtin_fmaf(w_use.y, raw[c & 3][1], w_use.x * raw[c & 3][0])));
        if (NS == 6) t = __builtin_fmaf(w2_use.y, raw[c & 3][NS - 1], __builtin_fmaf(w2_use.x, raw[c & 3][NS - 2], t));
        v[c] = t;
        asm("" : "+v"(v[c]));  // (scalar chains: see split3_bf16_pinned)
      };
      auto split_a = [&](int j) {
        ra[j] = v[2 * j];
        rb[j] = v[2 * j + 1];
        q1[j] = split_step_bf16_pinned(ra[j], rb[j]);
      };
      auto split_b = [&](int j) { q2[j] = split_step_bf16_pinned(ra[j], rb[j]); };
      auto split_c = [&](int j) { q3[j] = pack2(ra[j], rb[j]); };

#pragma unroll
      for (int p = 0; p < 3; ++p) anxt[p] = (wpa + (long long)nstep * MTW * 192)[(unsigned)(p * 64 + lane)];
      record((k + 3) % KT, o_next, w_next, o2_next, w2_next);
      MODE_SB
      MODE_MF(2, b0, 0) combine(0); MODE_SB
      MODE_MF(2, b0, 1) combine(1); MODE_SB
      MODE_MF(2, b0, 2) combine(2); MODE_SB
      MODE_MF(2, b0, 3) combine(3); MODE_SB
      words(wsrc, o_use, o2_use, 1);
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
      if (k < 4) {
        issue(chn, 2 * k, 2 * k);
        issue(chn, 2 * k + 1, 2 * k + 1);
      }
      MODE_SB
      MODE_MF(0, b1, 2) MODE_SB
      MODE_MF(0, b1, 3) MODE_SB
      // the record of the tap sampled under the NEXT tap becomes current; its first half batch of window words is requested here
      o_use = o_next;
      w_use = w_next;
      o2_use = o2_next;
      w2_use = w2_next;
#pragma unroll
      for (int gi = 0; gi < 4; ++gi) b0n[gi] = fnxt[(gi * 3 + 0) * 64];
      words(wsrcn, o_use, o2_use, 0);
      MODE_SB
      MODE_MF(0, b2, 0) MODE_SB
      if (k >= LAG && k < 4 + LAG) commit(chn, 2 * (k - LAG), 2 * (k - LAG), nxt);  // LAG taps after their loads were issued
      MODE_SB
      MODE_MF(0, b2, 1) MODE_SB
      if (k >= LAG && k < 4 + LAG) commit(chn, 2 * (k - LAG) + 1, 2 * (k - LAG) + 1, nxt);
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

  // D[i = c][j = pixel of group gset + gi]: written (this kernel owns every element of its tiles)
  const int hh = h0 + (wave / TW) * 32 + (lane & 31);
  const int cmax = d.Cog - mg * 128;
#pragma unroll
  for (int gi = 0; gi < 4; ++gi) {
    const int ww = w0 + gi;
    if (hh < d.H && ww < d.W) {
      float* yb = gx + ((long long)b * d.Co + (long long)g * d.Cog + (long long)mg * 128) * HW + (long long)hh * d.sh + (long long)ww * d.sw;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = MODE_ACC_ROW(m, r, half);
        if (co < cmax) yb[(long long)co * HW] = F16 ? acc[gi][r] * unscale : acc[gi][r];
      }
    }
  }
}

template <bool F16>
__global__ __launch_bounds__(NTHREADS) void sphere_bwd_data_split_kernel(const float* __restrict__ gy, const uint4* __restrict__ wps,
                                                                         float* __restrict__ gx, WinDims d, int NCH16,
                                                                         const int4* __restrict__ tiles, const int4* __restrict__ rec_off,
                                                                         const float4* __restrict__ rec_w, const int2* __restrict__ rec_off2,
                                                                         const float2* __restrict__ rec_w2, const float* __restrict__ amax_g,
                                                                         const float* __restrict__ amax_w) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float sx = 1.f, unscale = 1.f;
  if (F16) {
    sx = f16_scale_of(mode::absmax_load(amax_g));
    unscale = (1.f / sx) * (1.f / f16_scale_of(mode::absmax_load(amax_w)));
  }
  const int4 t = tiles[blockIdx.x];
  if ((t.w >> 16) == 0)
    bwd_data_tile<4, F16>(gy, wps, gx, d, NCH16, t, rec_off, rec_w, rec_off2, rec_w2, smem, sx, unscale);
  else
    bwd_data_tile<6, F16>(gy, wps, gx, d, NCH16, t, rec_off, rec_w, rec_off2, rec_w2, smem, sx, unscale);
}

// wps[(((((g*MG + mg)*NCH16 + ch)*KT + tap)*MTW + m)*3 + piece)*64 + lane] = 8 bf16: piece of W[o = g*Cog' + ch*16 + 8*(lane>>5) + j]
// [c = mg*128 + m*32 + (lane&31)][tap] -- the transposed weight: rows of this GEMM are the INPUT channels c of the layer, its reduction
// runs over the output channels o.  `d` carries the swapped roles (d.Cog = input channels per group, d.Cig = output channels per group).
template <bool F16>
__global__ void pack_w_win_split_t(const float* __restrict__ w, uint4* __restrict__ wps, WinDims d, int NCH16, const float* __restrict__ amax_w) {
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
    const int c = mg * 128 + m * 32 + (lane & 31);  // row of the GEMM = input channel of the layer (within the group)
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int o = ch * SP_CCH + 8 * (lane >> 5) + j;  // reduction index = output channel of the layer (within the group)
      v[j] = (c < d.Cog && o < d.Cig) ? w[((long long)(g * d.Cig + o) * d.Cog + c) * KT + tap] : 0.f;
      if (F16) v[j] *= sw;
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

}  // namespace

extern "C" size_t mode_sphere_conv_bwd_data_win_wpack_bytes(int Ci, int Co, int Kh, int Kw, int groups) {
  if (Ci <= 0 || Co <= 0 || groups <= 0 || Kh * Kw != KT || Ci % groups || Co % groups) return 0;
  const int Cig = Ci / groups, Cog = Co / groups;
  return (size_t)groups * mode::cdiv(Cig, 128) * mode::cdiv(Cog, SP_CCH) * KT * MTW * 3 * 64 * sizeof(uint4);
}

// 1 if the split kernel takes this layer: the reduction runs over the output channels of the layer in chunks of 16.
extern "C" int mode_sphere_conv_bwd_data_win_supported(int Ci, int Co, int groups) {
  return (Ci > 0 && Co > 0 && groups > 0 && Ci % groups == 0 && Co % groups == 0 && (Co / groups) % SP_CCH == 0) ? 1 : 0;
}

// gx (written, not added to) on the n_tiles good tiles of the adjoint plan; `transposed`: gy and gx are plane-transposed (B, C, W, H).
// The caller runs mode_sphere_conv_bwd_data_adj_list on the plan's bad tiles.
static int sphere_bwd_data_win_split(const char* who, const float* gy, const float* w, const float* amax_g, const float* amax_w, float* gx,
                                     float* wpack, const int32_t* tiles, int n_tiles, const int32_t* rec_off, const float* rec_w,
                                     const int32_t* rec_off2, const float* rec_w2, int B, int Ci, int H, int W, int Co, int Kh, int Kw,
                                     int groups, int transposed, mode_stream_t stream) {
  WinDims d;
  int rc = make_win_dims(d, B, Co, H, W, Ci, Kh, Kw, groups, who);  // roles swapped: this GEMM reduces over the layer's output channels
  if (rc != MODE_OK) return rc;
  MODE_REQUIRE(mode_sphere_conv_bwd_data_win_supported(Ci, Co, groups) == 1, MODE_ERR_UNSUPPORTED,
               "%s: the output channels per group (%d) must be a multiple of %d", who, Co / std::max(groups, 1), SP_CCH);
  MODE_REQUIRE(n_tiles >= 0 && (size_t)n_tiles <= mode_sphere_plan_max_tiles(H, W), MODE_ERR_BAD_ARG, "%s: bad tile count %d", who, n_tiles);
  if (transposed) {
    d.sh = 1;
    d.sw = H;
  }
  if (B == 0 || n_tiles == 0) return MODE_OK;
  MODE_REQUIRE(gy && w && gx && wpack && tiles && rec_off && rec_w && rec_off2 && rec_w2, MODE_ERR_BAD_ARG, "%s: null pointer", who);
  MODE_REQUIRE(B <= 65535 && d.G * d.MG <= 65535, MODE_ERR_UNSUPPORTED, "%s: grid limit", who);
  hipStream_t st = mode::as_stream(stream);
  const int NCH16 = d.Cig / SP_CCH;
  uint4* wps = reinterpret_cast<uint4*>(wpack);
  const long long nsplit = (long long)d.G * d.MG * NCH16 * KT * MTW * 64;
  if (mode::pack_needed()) {
    if (amax_g)
      hipLaunchKernelGGL(pack_w_win_split_t<true>, dim3(mode::cdiv(nsplit, 256)), dim3(256), 0, st, w, wps, d, NCH16, amax_w);
    else
      hipLaunchKernelGGL(pack_w_win_split_t<false>, dim3(mode::cdiv(nsplit, 256)), dim3(256), 0, st, w, wps, d, NCH16, amax_w);
  }
  return launch_win(who, amax_g ? sphere_bwd_data_split_kernel<true> : sphere_bwd_data_split_kernel<false>, dim3(n_tiles, B, d.G * d.MG),
                    SP3_LDS_BYTES, st, gy, wps, gx, d, NCH16, reinterpret_cast<const int4*>(tiles), reinterpret_cast<const int4*>(rec_off),
                    reinterpret_cast<const float4*>(rec_w), reinterpret_cast<const int2*>(rec_off2), reinterpret_cast<const float2*>(rec_w2),
                    amax_g, amax_w);
}

extern "C" int mode_sphere_conv_bwd_data_win_split(const float* gy, const float* w, float* gx, float* wpack, const int32_t* tiles,
                                                   int n_tiles, const int32_t* rec_off, const float* rec_w, const int32_t* rec_off2,
                                                   const float* rec_w2, int B, int Ci, int H, int W, int Co, int Kh, int Kw, int groups,
                                                   int transposed, mode_stream_t stream) {
  return sphere_bwd_data_win_split("mode_sphere_conv_bwd_data_win_split", gy, w, nullptr, nullptr, gx, wpack, tiles, n_tiles, rec_off, rec_w,
                                   rec_off2, rec_w2, B, Ci, H, W, Co, Kh, Kw, groups, transposed, stream);
}

// The same on the two-piece fp16 arithmetic (mode_sphere_conv_fwd_win_split_f16): amax_g / amax_w = the maximum buffers of gy and of w.
extern "C" int mode_sphere_conv_bwd_data_win_split_f16(const float* gy, const float* w, const float* amax_g, const float* amax_w, float* gx,
                                                       float* wpack, const int32_t* tiles, int n_tiles, const int32_t* rec_off,
                                                       const float* rec_w, const int32_t* rec_off2, const float* rec_w2, int B, int Ci, int H,
                                                       int W, int Co, int Kh, int Kw, int groups, int transposed, mode_stream_t stream) {
  MODE_REQUIRE(amax_g && amax_w, MODE_ERR_BAD_ARG, "mode_sphere_conv_bwd_data_win_split_f16: null maximum");
  return sphere_bwd_data_win_split("mode_sphere_conv_bwd_data_win_split_f16", gy, w, amax_g, amax_w, gx, wpack, tiles, n_tiles, rec_off, rec_w,
                                   rec_off2, rec_w2, B, Ci, H, W, Co, Kh, Kw, groups, transposed, stream);
}
