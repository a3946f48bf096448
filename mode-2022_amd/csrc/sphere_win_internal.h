// What the windowed spherical kernels share across their translation units: sphere_win_fwd.hip (forward), sphere_win_bww.hip (weight
// gradient) and sphere_win_bwd_data.hip (input gradient).  Included by those three files only; everything here sits in an
// anonymous namespace, so each file compiles its own copy and the kernels' symbols stay internal to their file.
//
// The sampling tables of the network are not arbitrary: a gnomonic kernel on an equirectangular grid is shift-invariant along the
// longitude axis, so all samples of a small block of output pixels fall into a compact window of the input (a few columns wide; a
// few rows taller than the block, except next to the poles where it wraps around the whole longitude axis).  The windowed kernels
// stage that window ONCE per channel chunk in LDS with plain row loads and build the MFMA operand on the fly from it.  Nothing is
// assumed about the table: the host plans every tile from the actual table values (mode_sphere_plan_build in sphere_plan.hip: same
// record arithmetic as the kernels, sphere_tap.h, same tile and window sizes, sphere_win_geometry.h) and classifies it by the
// window it needs.  A table whose tiles do not fit any window class is reported as such and the caller uses the general kernels
// of sphere_conv.hip.
#pragma once

#include <algorithm>

#include "common.h"
#include "bn_internal.h"
#include "sphere_internal.h"
#include "sphere_tap.h"
#include "sphere_win_geometry.h"
#include "split_arith.h"

namespace {

using namespace mode::split;
using namespace mode::sphere_win;  // TH, TW, WC, CCH, KT, NTHREADS, the window classes: what the planners share with the kernels

typedef float f32x32 __attribute__((ext_vector_type(32)));

constexpr int MTW = 4;     // M-tiles (32 output channels each) per wave

struct WinDims {
  int B, Ci, H, W, Co, G;
  int Cig, Cog;
  int NCH;  // channel chunks
  int MG;   // 128-channel output slices per group
  int wr;   // window rows of the wrap-around class (H + 1)
  int wrap_pipe;  // wrap-around class double-buffered (fits LDS and registers) or staged in place
  int sh, sw;     // element strides of h and w in the activation tensors: (W, 1) = NCHW; (1, H) = planes stored transposed
  int accumulate;
};

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// Row i of D (an output channel of the 128-channel slice) that register r of M-tile m holds in half-wave `half` (32 x 32 MFMA layout).
// (a macro: as an inlined function the same expression moved four selects in the eval epilogue of sphere_fwd_split_kernel)
#define MODE_ACC_ROW(m, r, half) ((m) * 32 + ((r) & 3) + 8 * ((r) >> 2) + 4 * (half))

// The small-window tiles on the split arithmetic (sphere_fwd_split_kernel, and sphere_bwd_data_split_kernel on the same structure): a
// chunk is 16 channels deep, its window of 81 rows x 8 columns per channel is fp32 and double-buffered, the sampled operand goes
// through operand buffers in LDS.
constexpr int SP_CCH = 16;
constexpr int SP_CP = chan_pitch(WR_SMALL);
constexpr int SP_WIN = SP_CCH * SP_CP;                      // floats per window buffer
constexpr int SP_WIN_FLOATS = ((2 * SP_WIN + WR_SMALL + 8 + 3) / 4) * 4;  // both buffers + slack, 16-byte multiple
constexpr int SP_OP = 8 * 3 * 64;                           // uint4 per operand buffer
constexpr size_t SP_LDS_BYTES = (size_t)SP_WIN_FLOATS * sizeof(float) + 2 * (size_t)SP_OP * sizeof(uint4);
constexpr size_t SP3_LDS_BYTES = SP_LDS_BYTES + (size_t)SP_OP * sizeof(uint4);  // the forward keeps three operand buffers
static_assert(SP3_LDS_BYTES <= 160 * 1024, "windows + three operand buffers must fit the 160 KB of a CU");

constexpr int TP = 5;  // tap pairs of a 3 x 3 kernel (the tall-window tiles of the split forward: K = 8 channels x 2 taps)

// the tall tiles of the split forward keep two pair steps of weight fragments (2 x 12 KB) behind their windows
constexpr size_t TALL_W_BYTES = 2 * (size_t)MTW * 3 * 64 * sizeof(uint4);
size_t tall_split_lds_bytes(int wr) { return ((win_lds_bytes(wr, true) + 15) / 16) * 16 + TALL_W_BYTES; }

int make_win_dims(WinDims& d, int B, int Ci, int H, int W, int Co, int Kh, int Kw, int groups, const char* who) {
  MODE_REQUIRE(B >= 0 && Ci > 0 && H > 0 && W > 0 && Co > 0 && groups > 0, MODE_ERR_BAD_ARG, "%s: non-positive size", who);
  MODE_REQUIRE(Kh * Kw == KT, MODE_ERR_UNSUPPORTED, "%s: the windowed kernels are built for %d taps (got %dx%d)", who, KT, Kh, Kw);
  MODE_REQUIRE(Ci % groups == 0 && Co % groups == 0, MODE_ERR_BAD_ARG, "%s: channels not divisible by groups", who);
  MODE_REQUIRE((long long)H * W < (1LL << 30), MODE_ERR_UNSUPPORTED, "%s: image too large", who);
  d.B = B; d.Ci = Ci; d.H = H; d.W = W; d.Co = Co; d.G = groups;
  d.Cig = Ci / groups;
  d.Cog = Co / groups;
  d.NCH = mode::cdiv(d.Cig, CCH);
  d.MG = mode::cdiv(d.Cog, 128);
  d.wr = H + 1;
  d.sh = W;
  d.sw = 1;
  d.wrap_pipe = wrap_is_pipelined(H) ? 1 : 0;
  d.accumulate = 0;
  return MODE_OK;
}

// Host: one launch of a kernel with dynamic LDS -- the opt-in above 64 KiB, the launch, the launch check.
template <typename... P, typename... A>
int launch_win(const char* who, void (*kernel)(P...), dim3 grid, size_t lds, hipStream_t st, A... args) {
  int rc = mode::allow_lds(kernel, lds, who);
  if (rc != MODE_OK) return rc;
  hipLaunchKernelGGL(kernel, grid, dim3(NTHREADS), lds, st, args...);
  return mode::check_launch(who);
}

// The slots of the hand-scheduled tap loops (sphere_fwd_split_kernel, fwd_tile_split, bwd_data_tile): a slot is one MFMA and the
// vector / LDS work placed beside it, closed by MODE_SB so that the compiler moves nothing across.  The MFMA macros name their
// user's locals: acc[], the weight fragments acur[piece] (small tiles) or a_cur[m][piece] (tall tiles), the operand pieces B / bq.
// The fp16 forms pin the MFMA to its slot with an empty asm that consumes the accumulator: without a consumer in the slot the
// compiler sinks the MFMAs below their sched_barriers, to where their operands' registers are assembled.
#define MODE_SB __builtin_amdgcn_sched_barrier(0);
#define MODE_MF(PA, B, gi) acc[gi] = mfma_bf16(acur[PA], B[gi], acc[gi]);
#define MODE_MFH(PA, B, gi) acc[gi] = mfma_f16(acur[PA], B[gi], acc[gi]); asm volatile("" :: "v"(acc[gi]));
#define MODE_TMF(PA, PB, m, t) acc[t] = mfma_bf16(a_cur[m][PA], bq[PB], acc[t]);
#define MODE_TMFH(PA, PB, m, t) acc[t] = mfma_f16(a_cur[m][PA], bq[PB], acc[t]); asm volatile("" :: "v"(acc[t]));

#ifdef MODE_TAPTIME
// debug build only (tools/experiments/sphere_taptime.py): s_memtime stamps of wave 0 of every small-window workgroup of the forward;
// sphere_win_fwd.hip defines the array and reads it back (mode_debug_taptime).  Inside this anonymous namespace the declaration has
// internal linkage, one array per file: only the forward file may stamp -- a MODE_STAMP in another file would not link.
extern __device__ unsigned long long g_taptime[8 * 8192];
#define MODE_STAMP(j) if (threadIdx.x == 0) g_taptime[((blockIdx.y * gridDim.x + blockIdx.x) & 8191) * 8 + (j)] = __builtin_readcyclecounter();
#define MODE_STAMPV(j, v) if (threadIdx.x == 0) g_taptime[((blockIdx.y * gridDim.x + blockIdx.x) & 8191) * 8 + (j)] = (v);
#else
#define MODE_STAMP(j)
#define MODE_STAMPV(j, v)
#endif

}  // namespace
