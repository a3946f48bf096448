// Tile and window geometry of the windowed spherical kernels, shared by the kernels (sphere_win_*.hip) and the host-side planners
// that cut a sampling table into their tiles (sphere_plan.hip): both sides must agree on every number here.
#pragma once
#include <cstddef>

namespace mode {
namespace sphere_win {

constexpr int RB = 2;      // MFMA N-tiles (32 rows) per tile column
constexpr int TH = 32 * RB;  // tile rows
constexpr int TW = 4;      // tile columns
constexpr int WC = 8;      // window columns
constexpr int CCH = 8;     // input channels per chunk
constexpr int KT = 9;      // taps (3x3 kernels)
constexpr int NTHREADS = 64 * TW * RB;  // one wave per (column, 32-row block)
constexpr int SROWS = NTHREADS / WC;    // window rows staged per pass
constexpr int WR_SMALL = TH + 17, WR_MID = TH + 81;  // window rows of the two compact classes (odd: conflict-free column pitch)
constexpr int WR_PIPE_MAX = 5 * SROWS;  // tallest window whose next chunk still fits in registers while the current one computes
constexpr int AJ_PIX = TH * TW;  // 256 pixels per tile = 8 waves x 32 lanes (the record order of the adjoint plan)
// The fp16 form of the windowed input gradient splits sx * G_k[o][q], G_k the sum of an adjoint list's weights times gy, with
// max |gy| sx < 2^15: the operand stays a finite fp16 number (<= 65504) whatever gy holds only while the list's weights sum to no more
// than 65504 / 2^15 = 2 - 2^-10.  The planner keeps a tile with a heavier list off the windowed kernel (a bad tile: fp32 gather).
constexpr float ADJ_F16_HEADROOM = 65504.f / 32768.f;

// weight gradient: a work item is one 32-row half of a tile column
constexpr int BW_TH = 32;                  // rows per work item
constexpr int BW_WR = BW_TH + 17;          // its window rows (49)
constexpr int BW_NREC = KT * BW_TH;        // records per column (288)
// ... next to the poles, one small window per tap (pitems[i] = (h0, w, rbase[9], cbase[9]))
constexpr int BP_WR = BW_TH + 2;         // rows per tap window
constexpr int BP_TAPW = 2 * BP_WR;       // floats per tap window: [2 cols][34 rows]
constexpr int BP_ITEM_INTS = 2 + 2 * KT;

#ifdef __HIPCC__
__host__ __device__
#endif
constexpr int chan_pitch(int wr) {
  // 8 columns of wr rows, padded so that consecutive channels are 32 banks apart (the two half-waves of a B read)
  return WC * wr + ((32 - (WC * wr) % 64) + 64) % 64;
}
// LDS bytes of the forward's window (double-buffered when `pipe`), and whether the wrap-around class is double-buffered at height H
constexpr size_t win_lds_bytes(int wr, bool pipe) { return ((size_t)(pipe ? 2 : 1) * CCH * chan_pitch(wr) + wr + 8) * sizeof(float); }
constexpr bool wrap_is_pipelined(int H) { return H + 1 <= WR_PIPE_MAX && win_lds_bytes(H + 1, true) <= 160 * 1024; }

}  // namespace sphere_win
}  // namespace mode
