// Host-side planners of the windowed spherical kernels (sphere_win_*.hip): they cut a sampling table into the tiles, windows and
// sampling records those kernels run on.  No kernel in here -- plain host code on host memory, with the record arithmetic the kernels use
// (sphere_tap.h) and their geometry (sphere_win_geometry.h).
#include <algorithm>
#include <cstring>
#include <vector>

#define MODE_HOST_ONLY  // no device helper, no kernel from common.h
#include "common.h"
#include "sphere_tap.h"
#include "sphere_win_geometry.h"

using namespace mode::sphere_win;

namespace {

// Class 0 also promises the weight-gradient kernel that each 32-row half of the tile fits a 49-row window starting at
// rbase (+32 for the second half): true for shift-invariant tables, checked for all.
bool halves_fit(const float* pos_host, int H, int W, int KK, int h0, int w0, int rbase, int cbase) {
  const long long HW = (long long)H * W;
  for (int hf = 0; hf < 2; ++hf) {
    const int rb = (rbase + hf * BW_TH) % H;
    for (int k = 0; k < KK; ++k)
      for (int h = h0 + hf * BW_TH; h < std::min(h0 + (hf + 1) * BW_TH, H); ++h)
        for (int w = w0; w < std::min(w0 + TW, W); ++w) {
          int r0, c0;
          float4 wt;
          const long long idx = (long long)h * W + w;
          if (!mode::tap_record_fixed(pos_host[(2 * k) * HW + idx], pos_host[(2 * k + 1) * HW + idx], H, W, r0, c0, wt)) continue;
          if (wt.x == 0.f && wt.y == 0.f && wt.z == 0.f && wt.w == 0.f) continue;
          const int lr = ((r0 - rb) % H + H) % H;
          if (lr + 1 >= BW_WR || c0 - cbase < 0 || c0 - cbase + 1 >= WC) return false;
        }
  }
  return true;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// Host-side tile plan.  tiles_host[4*i .. 4*i+3] = (h0, w0, rbase, cbase) ordered by class; counts[c] = tiles of class c:
//   0: window of 81 rows   1: 145 rows   2: all H rows + 1 (wraps around)   3: does not fit (caller must use the general path)
// and the class is also stored in bits 16.. of the 4th word (cbase | class << 16).
// Inside a class the tiles are ordered so that, with the round-robin workgroup -> XCD assignment, the tiles that share rows of
// the output (and cache lines of the input window) run on the same XCD and meet in its L2.
extern "C" size_t mode_sphere_plan_max_tiles(int H, int W) {
  if (H <= 0 || W <= 0) return 0;
  return (size_t)mode::cdiv(H, TH) * mode::cdiv(W, TW);
}

extern "C" int mode_sphere_plan_build(const float* pos_host, int H, int W, int Kh, int Kw, int32_t* tiles_host, int32_t* counts) {
  MODE_REQUIRE(pos_host && tiles_host && counts, MODE_ERR_BAD_ARG, "mode_sphere_plan_build: null pointer");
  MODE_REQUIRE(H > 0 && W > 0 && Kh > 0 && Kw > 0, MODE_ERR_BAD_ARG, "mode_sphere_plan_build: non-positive size");
  const int KK = Kh * Kw;
  const long long HW = (long long)H * W;
  const int nth = mode::cdiv(H, TH), ntw = mode::cdiv(W, TW);
  std::vector<int32_t> cls[4];
  // order: groups of 8 row-blocks; inside a group all column blocks; inside a column block the 8 row-blocks -> index % 8
  // (the XCD) is the row-block, for every column block
  for (int hg = 0; hg < nth; hg += kNumXCD)
    for (int tw = 0; tw < ntw; ++tw)
      for (int hs = 0; hs < kNumXCD && hg + hs < nth; ++hs) {
        const int h0 = (hg + hs) * TH, w0 = tw * TW;
        int dmin = 1 << 30, dmax = -(1 << 30), cmin = 1 << 30, cmax = -(1 << 30);
        bool any = false;
        for (int k = 0; k < KK; ++k)
          for (int h = h0; h < std::min(h0 + TH, H); ++h)
            for (int w = w0; w < std::min(w0 + TW, W); ++w) {
              int r0, c0;
              float4 wt;
              const long long idx = (long long)h * W + w;
              if (!mode::tap_record_fixed(pos_host[(2 * k) * HW + idx], pos_host[(2 * k + 1) * HW + idx], H, W, r0, c0, wt)) continue;
              if (wt.x == 0.f && wt.y == 0.f && wt.z == 0.f && wt.w == 0.f) continue;
              int dr = r0 - h0;  // wrapped into (-H/2, H/2]
              dr %= H;
              if (dr > H / 2) dr -= H;
              if (dr <= -(H + 1) / 2) dr += H;
              dmin = std::min(dmin, dr);
              dmax = std::max(dmax, dr);
              cmin = std::min(cmin, c0);
              cmax = std::max(cmax, c0);
              any = true;
            }
        int c = 0, rbase = h0, cbase = std::min(w0, std::max(W - WC, 0));
        if (any) {
          const int rows = dmax - dmin + 2;  // + the second corner row
          const int cols = cmax - cmin + 2;
          cbase = cmin;
          rbase = ((h0 + dmin) % H + H) % H;
          if (cols > WC) {
            c = 3;
          } else if (rows <= WR_SMALL && halves_fit(pos_host, H, W, KK, h0, w0, rbase, cbase)) {
            c = 0;
          } else if (rows <= WR_MID) {
            c = 1;
          } else {
            c = 2;  // whole axis: any start works, take 0 so that no row index wraps twice
            rbase = 0;
            if (win_lds_bytes(H + 1, false) > 160 * 1024) c = 3;
          }
        }
        if (cbase >= (1 << 16)) c = 3;
        cls[c].insert(cls[c].end(), {h0, w0, rbase, cbase | (c << 16)});
      }
  size_t o = 0;
  for (int c = 0; c < 4; ++c) counts[c] = (int32_t)(cls[c].size() / 4);
  for (int c : {2, 1, 0, 3}) {  // tall windows first: they are the slowest tiles of the launch
    if (!cls[c].empty()) std::memcpy(tiles_host + o, cls[c].data(), cls[c].size() * sizeof(int32_t));
    o += cls[c].size();
  }
  return MODE_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Pixels of the tiles that are NOT of the small-window class, sorted by linear index (they go to the general kernels).
extern "C" int mode_sphere_plan_rest_pixels(const int32_t* tiles_host, const int32_t* counts, int H, int W, int32_t* pix_host,
                                            int32_t* n_pix) {
  MODE_REQUIRE(tiles_host && counts && pix_host && n_pix, MODE_ERR_BAD_ARG, "mode_sphere_plan_rest_pixels: null pointer");
  const int n = counts[0] + counts[1] + counts[2] + counts[3];
  std::vector<int32_t> v;
  for (int i = 0; i < n; ++i) {
    const int32_t* t = tiles_host + 4 * i;
    if ((t[3] >> 16) == 0) continue;
    for (int h = t[0]; h < std::min(t[0] + TH, H); ++h)
      for (int w = t[1]; w < std::min(t[1] + TW, W); ++w) v.push_back(h * W + w);
  }
  std::sort(v.begin(), v.end());
  if (!v.empty()) std::memcpy(pix_host, v.data(), v.size() * sizeof(int32_t));
  *n_pix = (int32_t)v.size();
  return MODE_OK;
}

// Sampling records of the small-window tiles for the weight-gradient kernel, in tile-list order:
//   index (((ti*2 + half)*4 + column)*9 + tap)*32 + row -> window offset (rec_off) and the 4 corner weights (rec_w, 4 floats)
extern "C" size_t mode_sphere_plan_records_count(int n_small) { return n_small > 0 ? (size_t)n_small * 2 * TW * BW_NREC : 0; }

extern "C" int mode_sphere_plan_records(const float* pos_host, const int32_t* tiles_host, const int32_t* counts, int H, int W,
                                        float* rec_w_host, int32_t* rec_off_host) {
  MODE_REQUIRE(pos_host && tiles_host && counts && rec_w_host && rec_off_host, MODE_ERR_BAD_ARG, "mode_sphere_plan_records: null pointer");
  const long long HW = (long long)H * W;
  const int32_t* small = tiles_host + 4 * (size_t)(counts[2] + counts[1]);  // list order: wrap-around, mid, small
  for (int ti = 0; ti < counts[0]; ++ti) {
    const int h0 = small[4 * ti], w0 = small[4 * ti + 1], rbase = small[4 * ti + 2], cbase = small[4 * ti + 3] & 0xffff;
    for (int hf = 0; hf < 2; ++hf) {
      const int rb = (rbase + hf * BW_TH) % H;
      for (int wc = 0; wc < TW; ++wc)
        for (int k = 0; k < KT; ++k)
          for (int px = 0; px < BW_TH; ++px) {
            const size_t o = ((((size_t)ti * 2 + hf) * TW + wc) * KT + k) * BW_TH + px;
            const int h = h0 + hf * BW_TH + px, w = w0 + wc;
            int r0 = 0, c0 = 0;
            float4 wt = make_float4(0.f, 0.f, 0.f, 0.f);
            bool live = false;
            if (h < H && w < W) {
              const long long idx = (long long)h * W + w;
              live = mode::tap_record_fixed(pos_host[(2 * k) * HW + idx], pos_host[(2 * k + 1) * HW + idx], H, W, r0, c0, wt);
            }
            live = live && !(wt.x == 0.f && wt.y == 0.f && wt.z == 0.f && wt.w == 0.f);
            rec_off_host[o] = live ? (c0 - cbase) * BW_WR + ((r0 - rb) % H + H) % H : 0;
            rec_w_host[4 * o + 0] = live ? wt.x : 0.f;
            rec_w_host[4 * o + 1] = live ? wt.y : 0.f;
            rec_w_host[4 * o + 2] = live ? wt.z : 0.f;
            rec_w_host[4 * o + 3] = live ? wt.w : 0.f;
          }
    }
  }
  return MODE_OK;
}

// Work items of the polar weight-gradient kernel: every tile that is NOT of the small-window class, split into 2 halves x 4
// columns.  pitems_host[20 * i ..] = (h0, w, rbase[9], cbase[9]); rec_w_host[4 * (i*288 + tap*32 + row)], rec_off_host[...] = the
// sampling records in the per-tap window layout.  Returns the number of items, or -1 (in *n_items) if some column does not fit
// its per-tap windows (34 rows x 2 columns per tap) -- the caller then keeps those pixels on the general kernel.
extern "C" size_t mode_sphere_plan_polar_max_items(const int32_t* counts) {
  return counts ? (size_t)(counts[1] + counts[2]) * 2 * TW : 0;
}

extern "C" int mode_sphere_plan_polar(const float* pos_host, const int32_t* tiles_host, const int32_t* counts, int H, int W,
                                      int32_t* pitems_host, float* rec_w_host, int32_t* rec_off_host, int32_t* n_items) {
  MODE_REQUIRE(pos_host && tiles_host && counts && pitems_host && rec_w_host && rec_off_host && n_items, MODE_ERR_BAD_ARG,
               "mode_sphere_plan_polar: null pointer");
  const long long HW = (long long)H * W;
  const int ntall = counts[2] + counts[1];  // list order: wrap-around, mid, small
  int ni = 0;
  for (int ti = 0; ti < ntall; ++ti) {
    const int th0 = tiles_host[4 * ti], tw0 = tiles_host[4 * ti + 1];
    for (int hf = 0; hf < 2; ++hf)
      for (int wc = 0; wc < TW; ++wc) {
        const int h0 = th0 + hf * BW_TH, w = tw0 + wc;
        if (h0 >= H || w >= W) continue;
        int32_t* pi = pitems_host + (size_t)ni * BP_ITEM_INTS;
        pi[0] = h0;
        pi[1] = w;
        for (int k = 0; k < KT; ++k) {
          // row SHIFT of every live pixel, n = r0 - (h0 + px) modulo H, taken relative to the first one so that a shift of about
          // half the axis (the far side of the sphere) does not straddle the wrap-around cut
          int nfirst = 0, nmin = 1 << 30, nmax = -(1 << 30), cmin = 1 << 30, cmax = -(1 << 30);
          bool have = false;
          for (int px = 0; px < BW_TH && h0 + px < H; ++px) {
            int r0, c0;
            float4 wt;
            const long long idx = (long long)(h0 + px) * W + w;
            if (!mode::tap_record_fixed(pos_host[(2 * k) * HW + idx], pos_host[(2 * k + 1) * HW + idx], H, W, r0, c0, wt)) continue;
            if (wt.x == 0.f && wt.y == 0.f && wt.z == 0.f && wt.w == 0.f) continue;
            int n = ((r0 - h0 - px) % H + H) % H;
            if (!have) {
              nfirst = n;
              have = true;
            }
            n = ((n - nfirst + H / 2) % H + H) % H - H / 2 + nfirst;  // within H/2 of the first shift
            nmin = std::min(nmin, n);
            nmax = std::max(nmax, n);
            cmin = std::min(cmin, c0);
            cmax = std::max(cmax, c0);
          }
          int rb = 0, cbs = 0;
          if (have) {
            // rows h0 + nmin .. h0 + 31 + nmax (+1 for the second corner) must fit the 34-row window, the columns its 2
            if (BW_TH - 1 + (nmax - nmin) + 2 > BP_WR || cmax - cmin + 2 > 2) {
              *n_items = -1;
              return MODE_OK;
            }
            rb = ((h0 + nmin) % H + H) % H;
            cbs = cmin;
          }
          pi[2 + k] = rb;
          pi[2 + KT + k] = cbs;
          for (int px = 0; px < BW_TH; ++px) {
            const size_t o = ((size_t)ni * KT + k) * BW_TH + px;
            int r0 = 0, c0 = 0;
            float4 wt = make_float4(0.f, 0.f, 0.f, 0.f);
            bool live = false;
            if (h0 + px < H) {
              const long long idx = (long long)(h0 + px) * W + w;
              live = mode::tap_record_fixed(pos_host[(2 * k) * HW + idx], pos_host[(2 * k + 1) * HW + idx], H, W, r0, c0, wt);
            }
            live = live && !(wt.x == 0.f && wt.y == 0.f && wt.z == 0.f && wt.w == 0.f);
            rec_off_host[o] = live ? k * BP_TAPW + (c0 - cbs) * BP_WR + ((r0 - rb) % H + H) % H : 0;
            rec_w_host[4 * o + 0] = live ? wt.x : 0.f;
            rec_w_host[4 * o + 1] = live ? wt.y : 0.f;
            rec_w_host[4 * o + 2] = live ? wt.z : 0.f;
            rec_w_host[4 * o + 3] = live ? wt.w : 0.f;
          }
        }
        ++ni;
      }
  }
  *n_items = ni;
  return MODE_OK;
}

// Host-side plan of the adjoint windows (stride 1, output grid = input grid).  For every 64 x 4 tile of INPUT pixels q (same tiling as
// mode_sphere_plan_build) it collects L(k, q) for all nine taps and all pixels of the tile.  A tile is "good" when every list has at
// most 6 entries whose weights sum to no more than ADJ_F16_HEADROOM = 2 - 2^-10 (sphere_win_geometry.h: what keeps the fp16 form's
// scaled operand finite; next to a pole of a small table six output pixels crowd onto one source with a sum of 2.18) and all their
// source pixels lie in one window of WR_SMALL rows x WC columns:
//   good_tiles[4 i ..] = (h0, w0, rbase, cbase | six << 16), six = 1 when some list of the tile has 5 or 6 entries (slots 4, 5 in
//   rec_off2 / rec_w2 [((i * 9 + tap) * 256 + pixel) * 2 + slot - 4]; lists longer than 6 make a tile bad);
//   rec_off / rec_w [((i * 9 + tap) * 256 + pixel) * 4 + slot], pixel =
//   ((rowblock * 4 + column) * 32 + row) -- the lane order of the kernel; offset = (source column - cbase) * WR_SMALL + (source row -
//   rbase) mod H, unused slots (0, 0.0f); slots in ascending source-pixel order (the gather kernel's summation order).
//   bad_tiles[2 j ..] = (h0, w0) of the others.  counts = (good, bad).
// A tile that qualifies but for a list heavier than the headroom is a BAD tile (listed, counted).  Its entry and records are written all
// the same, behind those of the counts[0] good tiles, with bit 17 of the fourth word set: the three-piece bf16 form has no headroom
// to keep and may take them (mode_hip/functional.py does, after clearing the bit); the fp16 form must not.
extern "C" int mode_sphere_adjplan_build(const float* pos_host, int H, int W, int Kh, int Kw, int32_t* good_tiles, int32_t* bad_tiles,
                                         int32_t* counts, int32_t* rec_off_host, float* rec_w_host, int32_t* rec_off2_host,
                                         float* rec_w2_host) {
  MODE_REQUIRE(pos_host && good_tiles && bad_tiles && counts && rec_off_host && rec_w_host && rec_off2_host && rec_w2_host,
               MODE_ERR_BAD_ARG, "mode_sphere_adjplan_build: null pointer");
  MODE_REQUIRE(H > 0 && W > 0 && Kh * Kw == KT, MODE_ERR_BAD_ARG, "mode_sphere_adjplan_build: needs a positive size and %d taps", KT);
  const long long HW = (long long)H * W;
  MODE_REQUIRE((long long)KT * HW * 4 < (1ll << 31), MODE_ERR_UNSUPPORTED, "mode_sphere_adjplan_build: table too large");
  // adjoint lists in CSR form, rows (tap, q), filled in ascending p (the order of mode_sphere_adjoint_build)
  std::vector<int32_t> rowptr((size_t)KT * HW + 1, 0);
  auto corners = [&](int k, long long p, int qs[4], float ws[4]) -> int {
    const float h = pos_host[(long long)(2 * k) * HW + p], w = pos_host[(long long)(2 * k + 1) * HW + p];
    if (!(h > -1.f && w > -1.f && h < (float)H && w < (float)W)) return 0;
    const float hf = floorf(h), wf = floorf(w);
    const int hl = (int)hf, wl = (int)wf, hh = hl + 1, wh = wl + 1;
    const float lh = h - hf, lw = w - wf, uh = 1.f - lh, uw = 1.f - lw;
    const float wt[4] = {uh * uw, uh * lw, lh * uw, lh * lw};
    const int hc[4] = {hl, hl, hh, hh}, wc[4] = {wl, wh, wl, wh};
    int n = 0;
    for (int i = 0; i < 4; ++i)
      if (hc[i] >= 0 && hc[i] <= H - 1 && wc[i] >= 0 && wc[i] <= W - 1 && wt[i] != 0.f) {
        qs[n] = hc[i] * W + wc[i];
        ws[n] = wt[i];
        ++n;
      }
    return n;
  };
  int qs[4];
  float ws[4];
  for (int k = 0; k < KT; ++k)
    for (long long p = 0; p < HW; ++p) {
      const int n = corners(k, p, qs, ws);
      for (int i = 0; i < n; ++i) rowptr[(size_t)k * HW + qs[i] + 1]++;
    }
  for (size_t i = 0; i < (size_t)KT * HW; ++i) rowptr[i + 1] += rowptr[i];
  std::vector<int32_t> ep(rowptr.back());
  std::vector<float> ew(rowptr.back());
  {
    std::vector<int32_t> cur(rowptr.begin(), rowptr.end() - 1);
    for (int k = 0; k < KT; ++k)
      for (long long p = 0; p < HW; ++p) {
        const int n = corners(k, p, qs, ws);
        for (int i = 0; i < n; ++i) {
          const int32_t at = cur[(size_t)k * HW + qs[i]]++;
          ep[at] = (int32_t)p;
          ew[at] = ws[i];
        }
      }
  }
  const int nth = mode::cdiv(H, TH), ntw = mode::cdiv(W, TW);
  int ngood = 0, nbad = 0;
  struct GoodTile {
    int h0, w0, rbase, cbase, six;
  };
  std::vector<GoodTile> good, heavy_tiles;
  for (int hg = 0; hg < nth; hg += kNumXCD)  // tile order as in mode_sphere_plan_build (tiles sharing rows meet on one XCD)
    for (int tw = 0; tw < ntw; ++tw)
      for (int hs = 0; hs < kNumXCD && hg + hs < nth; ++hs) {
        const int h0 = (hg + hs) * TH, w0 = tw * TW;
        bool ok = h0 + TH <= H && w0 + TW <= W;  // whole tiles only: ragged edges stay on the gather kernel
        bool six = false;                        // some list has 5 or 6 entries: the 6-slot class
        bool heavy = false;                      // some list weighs more than the fp16 form's headroom
        int dmin = 1 << 30, dmax = -(1 << 30), cmin = 1 << 30, cmax = -(1 << 30);
        for (int k = 0; k < KT && ok; ++k)
          for (int h = h0; h < h0 + TH && ok; ++h)
            for (int w = w0; w < w0 + TW; ++w) {
              const size_t row = (size_t)k * HW + (size_t)h * W + w;
              const int nent = rowptr[row + 1] - rowptr[row];
              if (nent > 6) {
                ok = false;
                break;
              }
              if (nent > 4) six = true;
              double wsum = 0.0;  // (weights are products of numbers in [0, 1]: non-negative)
              for (int e = rowptr[row]; e < rowptr[row + 1]; ++e) wsum += (double)ew[e];
              if (wsum > (double)ADJ_F16_HEADROOM) heavy = true;
              for (int e = rowptr[row]; e < rowptr[row + 1]; ++e) {
                const int hp = ep[e] / W, wp = ep[e] % W;
                int dr = (hp - h0) % H;
                if (dr > H / 2) dr -= H;
                if (dr <= -(H + 1) / 2) dr += H;
                dmin = std::min(dmin, dr);
                dmax = std::max(dmax, dr);
                cmin = std::min(cmin, wp);
                cmax = std::max(cmax, wp);
              }
            }
        int rbase = h0, cbase = std::min(w0, std::max(W - WC, 0));
        if (ok && dmax >= dmin) {
          if (dmax - dmin + 1 > WR_SMALL || cmax - cmin + 1 > WC || cmin >= (1 << 16)) ok = false;
          rbase = ((h0 + dmin) % H + H) % H;
          cbase = cmin;
        }
        if (!ok) {
          bad_tiles[2 * nbad] = h0;
          bad_tiles[2 * nbad + 1] = w0;
          ++nbad;
          continue;
        }
        if (heavy) {  // a bad tile for whoever follows counts; its records are kept behind the good tiles' (below)
          bad_tiles[2 * nbad] = h0;
          bad_tiles[2 * nbad + 1] = w0;
          ++nbad;
          heavy_tiles.push_back({h0, w0, rbase, cbase, six ? 1 : 0});
          continue;
        }
        good.push_back({h0, w0, rbase, cbase, six ? 1 : 0});
      }
  // the 6-slot tiles first: they are the slowest workgroups of the launch, and started first they end inside its last round
  std::stable_sort(good.begin(), good.end(), [](const GoodTile& a, const GoodTile& b2) { return a.six > b2.six; });
  const size_t nlight = good.size();
  good.insert(good.end(), heavy_tiles.begin(), heavy_tiles.end());
  for (size_t gi = 0; gi < good.size(); ++gi) {
    const GoodTile& gt = good[gi];
    const int h0 = gt.h0, w0 = gt.w0, rbase = gt.rbase, cbase = gt.cbase;
    int32_t* tl = good_tiles + 4 * (size_t)ngood;
    tl[0] = h0; tl[1] = w0; tl[2] = rbase; tl[3] = cbase | (gt.six << 16) | (gi >= nlight ? 1 << 17 : 0);
    for (int k = 0; k < KT; ++k)
      for (int pix = 0; pix < AJ_PIX; ++pix) {
        const int wv = pix >> 5, h = h0 + (wv / TW) * 32 + (pix & 31), w = w0 + (wv % TW);
        const size_t row = (size_t)k * HW + (size_t)h * W + w;
        const size_t o = (((size_t)ngood * KT + k) * AJ_PIX + pix) * 4, o2 = o / 2;
        for (int s = 0; s < 4; ++s) {
          rec_off_host[o + s] = 0;
          rec_w_host[o + s] = 0.f;
        }
        rec_off2_host[o2] = rec_off2_host[o2 + 1] = 0;
        rec_w2_host[o2] = rec_w2_host[o2 + 1] = 0.f;
        int s = 0;
        for (int e = rowptr[row]; e < rowptr[row + 1]; ++e, ++s) {
          const int hp = ep[e] / W, wp = ep[e] % W;
          const int off = (wp - cbase) * WR_SMALL + ((hp - rbase) % H + H) % H;
          if (s < 4) {
            rec_off_host[o + s] = off;
            rec_w_host[o + s] = ew[e];
          } else {
            rec_off2_host[o2 + s - 4] = off;
            rec_w2_host[o2 + s - 4] = ew[e];
          }
        }
      }
    ++ngood;
  }
  counts[0] = (int32_t)nlight;  // (ngood - nlight heavy tiles follow, bit 17 set: not good tiles for the kernels as they stand)
  counts[1] = nbad;
  return MODE_OK;
}
