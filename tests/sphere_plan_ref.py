"""An interpreter of the plans of the windowed spherical kernels, in plain numpy.  TEST INFRASTRUCTURE.

`check_plan(table, plan, aplan)` takes a sampling table (1, 18, H, W) and the records HF.sphere_plan / HF.sphere_adjplan return for it,
and evaluates them the way the KERNELS consume them -- the indexing is read from csrc/sphere_win_fwd.hip, sphere_win_bww.hip and
sphere_win_bwd_data.hip (which window word a record offset names, which image pixel that word was staged from), not from the planners of
csrc/sphere_plan.hip, and no code of csrc/ runs here.  One channel, float64 sums over the plan's float32 weights.

What a kernel does with a plan, restated:

  forward (fwd_tile and its split twins)     tile (h0, w0, rbase, cbase | class << 16): a window of WR rows x 8 columns, WR = 81, 145 or
      H + 1 by class; window word (row r, column c) = x[(rbase + r) % H, cbase + c], zero where cbase + c >= W.  Every lane computes the
      record of its own (pixel, tap) from the table (first corner (r0, c0), four weights) and reads the words (lr, lc), (lr, lc + 1),
      (lr + 1, lc), (lr + 1, lc + 1) with lr = r0 - rbase (+ H when negative), lc = c0 - cbase.
  weight gradient, compact tiles             work item = a 32-row half `hf` of a compact tile: window of 49 rows x 8 columns from row
      (rbase + 32 hf) % H; record ((((tile * 2 + hf) * 4 + column) * 9 + tap) * 32 + row) = (offset, 4 weights); the kernel reads the
      words offset, offset + 49 (next column), offset + 1 (next row), offset + 50 of the layout [column][row].
  weight gradient, polar items               item (h0, w, rbase[9], cbase[9]) = 32 rows of one column of a tall-window tile: nine windows
      of 34 rows x 2 columns, one per tap, in the layout [tap][column][row]; record ((item * 9 + tap) * 32 + row); words offset,
      offset + 34, offset + 1, offset + 35; word (tap t, column c, row r) = x[(rbase[t] + r) % H, cbase[t] + c] (zero beyond W).
      Without polar items the pixels of the tall-window tiles are the plan's sorted pixel list (general kernel).
  input gradient (bwd_data_tile)             good tile (h0, w0, rbase, cbase | six << 16): a window of 81 rows x 8 columns of gy; record
      ((tile * 9 + tap) * 256 + pixel), pixel = ((row block * 4 + column) * 32 + row): four (offset, weight) slots, and two more that the
      kernel reads ONLY when the six flag is set; gx[q] = sum over taps and slots of weight * gcol[tap][window word].  The other tiles
      are 64-pixel runs of the plane-transposed storage, listed by id, for the gather kernel.

The checks: the structure (every tile once, classes against counts and list order, every pixel covered once, every corner with a
non-zero weight inside the window its consumer stages, the six flag, the list lengths) and the values against the float64 oracle
(oracle/sphere_conv_ref.py im2col / col2im_scatter).  The plan's weights are float32 -- 1 - l and the product are three roundings, a
relative 3 * 2^-24, rounded up to 2^-22 for the second-order terms; the oracle forms its weights in float64 from the same float32
coordinates.  Every failure is a PlanError (an AssertionError)."""
import numpy as np
import torch

from oracle import sphere_conv_ref

TH, TW, WC, KT = 64, 4, 8, 9  # csrc/sphere_win_geometry.h, restated
WR_SMALL, WR_MID = TH + 17, TH + 81
BW_TH, BW_WR = 32, 32 + 17
BP_WR = 32 + 2
BP_TAPW = 2 * BP_WR
BP_ITEM_INTS = 2 + 2 * KT
AJ_PIX = TH * TW
CCH = 8
LDS_LIMIT = 160 * 1024
CORNERS = ((0, 0), (0, 1), (1, 0), (1, 1))  # (row step, column step) of the weights x, y, z, w of a record
EPS = 2.0**-22


class PlanError(AssertionError):
  pass


def _require(ok, what, *args):
  if not ok:
    raise PlanError(what % args if args else what)


def chan_pitch(wr):
  return WC * wr + ((32 - (WC * wr) % 64) + 64) % 64


def win_lds_bytes(wr, pipe):
  """LDS bytes of the forward's window of wr rows (sphere_win_geometry.h win_lds_bytes, restated)."""
  return ((2 if pipe else 1) * CCH * chan_pitch(wr) + wr + 8) * 4


def tap_records(table):
  """The record every lane of the forward computes for its (pixel, tap) from the table (csrc/sphere_tap.h tap_record_fixed, restated in
  float32): (r0, c0 int arrays (9, H, W), weights float32 (9, H, W, 4), live bool (9, H, W)); live = a tap with some non-zero weight."""
  t = np.asarray(table, dtype=np.float32)[0]
  H, W = t.shape[1:]
  h, w = t[0::2], t[1::2]
  with np.errstate(invalid='ignore'):
    inside = (h > -1) & (w > -1) & (h < H) & (w < W)  # (NaN compares false: a dead tap)
  hs, ws = np.where(inside, h, np.float32(0)), np.where(inside, w, np.float32(0))
  hf, wf = np.floor(hs), np.floor(ws)
  hl, wl = hf.astype(np.int64), wf.astype(np.int64)
  lh, lw = hs - hf, ws - wf
  uh, uw = np.float32(1) - lh, np.float32(1) - lw
  zero = np.float32(0)
  tl = np.where((hl >= 0) & (wl >= 0), uh * uw, zero)
  tr = np.where((hl >= 0) & (wl + 1 <= W - 1), uh * lw, zero)
  bl = np.where((hl + 1 <= H - 1) & (wl >= 0), lh * uw, zero)
  br = np.where((hl + 1 <= H - 1) & (wl + 1 <= W - 1), lh * lw, zero)
  up = hl < 0  # rows -1 | 0: only the lower row exists, it moves to the first slot
  tl, tr, bl, br = np.where(up, bl, tl), np.where(up, br, tr), np.where(up, zero, bl), np.where(up, zero, br)
  left = wl < 0
  tl, bl, tr, br = np.where(left, tr, tl), np.where(left, br, bl), np.where(left, zero, tr), np.where(left, zero, br)
  wt = np.stack([tl, tr, bl, br], -1).astype(np.float32) * inside[..., None]
  live = inside & (wt != 0).any(-1)
  r0 = np.where(live, np.maximum(hl, 0), 0)
  c0 = np.where(live, np.maximum(wl, 0), 0)
  return r0, c0, wt * live[..., None], live


def adjoint_list_lengths(table):
  """(9, H, W) int: the number of (output pixel, corner) pairs with a non-zero float32 weight that land on input pixel q under tap k --
  the length of the adjoint list L(k, q), counted from the table alone."""
  r0, c0, wt, live = tap_records(table)
  H, W = r0.shape[1:]
  n = np.zeros((KT, H * W), dtype=np.int64)
  for i, (dr, dc) in enumerate(CORNERS):
    nz = wt[..., i] != 0
    q = (r0 + dr) * W + (c0 + dc)
    for k in range(KT):
      n[k] += np.bincount(q[k][nz[k]], minlength=H * W)
  return n.reshape(KT, H, W)


def tile_rows(table):
  """{(h0, w0): rows}: the rows (second corner row included) the live taps of every 64 x 4 tile span along the cyclic row axis, measured
  as the planner's classes are defined -- 0 for a tile without a live tap.  For tests that ask WHY a tile has its class."""
  r0, _, _, live = tap_records(table)
  H, W = r0.shape[1:]
  out = {}
  for h0 in range(0, H, TH):
    for w0 in range(0, W, TW):
      sl = (slice(None), slice(h0, h0 + TH), slice(w0, w0 + TW))
      if not live[sl].any():
        out[(h0, w0)] = 0
        continue
      d = (r0[sl][live[sl]] - h0) % H
      d = np.where(d > H // 2, d - H, d)
      out[(h0, w0)] = int(d.max() - d.min() + 2)
  return out


def _np(t):
  return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _window_read(x, rb, cb, e, wr, W):
  """x at the image pixel window word e of a [column][row] window of wr rows, based at (rb, cb), was staged from (zero beyond W)."""
  H = x.shape[0]
  col, row = e // wr, e % wr
  gc = cb + col
  return np.where(gc < W, x[(rb + row) % H, np.minimum(gc, W - 1)], 0.0)


# ------------------------------------------------------------------------------------------------ forward / weight-gradient plan
def check_tiles(table, plan):
  """Structure of the tile list; returns (tiles (n, 4) int64 with the class bits removed, class per tile)."""
  H, W = table.shape[2:]
  tiles, counts = _np(plan.tiles).astype(np.int64).reshape(-1, 4), plan.counts
  n0, n1, n2 = counts
  nth, ntw = -(-H // TH), -(-W // TW)
  _require(n0 + n1 + n2 == nth * ntw and tiles.shape[0] >= nth * ntw, 'counts %s do not add up to the %d x %d tile grid', counts, nth, ntw)
  tiles = tiles[:nth * ntw].copy()
  cls = tiles[:, 3] >> 16
  want = np.concatenate([np.full(n2, 2), np.full(n1, 1), np.full(n0, 0)])  # list order: wrap, mid, compact
  _require((cls == want).all(), 'class bits disagree with counts %s / the list order wrap, mid, compact at list positions %s', counts,
           np.nonzero(cls != want)[0][:8])
  tiles[:, 3] &= 0xffff
  _require((tiles[:, 0] % TH == 0).all() and (tiles[:, 1] % TW == 0).all() and (tiles[:, 0] >= 0).all() and (tiles[:, 0] < H).all() and
           (tiles[:, 1] >= 0).all() and (tiles[:, 1] < W).all(), 'a tile origin off the 64 x 4 grid')
  ids = tiles[:, 0] // TH * ntw + tiles[:, 1] // TW
  _require(len(np.unique(ids)) == nth * ntw, 'some tile of the grid is missing or listed twice')
  _require((tiles[:, 2] >= 0).all() and (tiles[:, 2] < H).all(), 'a window base row outside [0, H)')
  if n2:
    _require(win_lds_bytes(H + 1, False) <= LDS_LIMIT, 'wrap-around tiles whose window of %d rows does not fit the LDS', H + 1)
  return tiles, cls


def sample_forward(table, plan, x):
  """col (9, H, W) float64 as the forward kernels sample x (H, W) on this plan; every corner with a non-zero weight inside its window."""
  H, W = x.shape
  tiles, cls = check_tiles(table, plan)
  r0, c0, wt, live = tap_records(table)
  rb, cb, wr = (np.zeros((H, W), dtype=np.int64) for _ in range(3))
  for (h0, w0, rbase, cbase), c in zip(tiles, cls):
    rb[h0:h0 + TH, w0:w0 + TW], cb[h0:h0 + TH, w0:w0 + TW] = rbase, cbase
    wr[h0:h0 + TH, w0:w0 + TW] = (WR_SMALL, WR_MID, H + 1)[c]
  lr = r0 - rb
  lr = np.where(lr < 0, lr + H, lr)
  lc = c0 - cb
  col = np.zeros((KT, H, W))
  for i, (dr, dc) in enumerate(CORNERS):
    nz = wt[..., i] != 0
    ok = (lr + dr < wr) & (lc + dc >= 0) & (lc + dc < WC)
    if (nz & ~ok).any():
      k, h, w = (int(v[0]) for v in np.nonzero(nz & ~ok))
      raise PlanError('forward: corner %d of tap %d at pixel (%d, %d) is window word (row %d, column %d) of a %d x %d window' %
                      (i, k, h, w, lr[k, h, w] + dr, lc[k, h, w] + dc, wr[h, w], WC))
    e = np.where(nz, (lc + dc) * wr + lr + dr, 0)
    col += np.where(nz, wt[..., i].astype(np.float64) * _window_read(x, rb, cb, e, wr, W), 0.0)
  return col


def sample_records(table, plan, x):
  """(col (9, H, W) float64, covered (H, W) int) as the weight-gradient kernels sample x through the plan's records: the compact tiles'
  and the polar items'.  covered counts who covers a pixel: a compact record column, a polar item, or -- without polar items -- the
  pixel list."""
  H, W = x.shape
  tiles, cls = check_tiles(table, plan)
  n0, n1, n2 = plan.counts
  rest, nrest, rec_w, rec_off, polar = plan.rest, plan.nrest, _np(plan.rec_w), _np(plan.rec_off).astype(np.int64), plan.polar
  col = np.zeros((KT, H, W))
  covered = np.zeros((H, W), dtype=np.int64)

  def run(off, wts, rb, cb, wrp, lo, nwords, hh, ww, k, who):
    """records (offsets `off`, weights `wts` (..., 4)) of pixels (hh, ww) and taps k, on windows of `nwords` words that start at word
    `lo` of the layout and are based at (rb, cb) in the image."""
    inimg = (hh < H) & (ww < W)
    for i, (dr, dc) in enumerate(CORNERS):
      nz = (wts[..., i] != 0) & inimg
      e = off + dc * wrp + dr
      ok = (off >= lo) & ((off - lo) % wrp + dr < wrp) & (e < lo + nwords)
      if (nz & ~ok).any():
        at = tuple(int(v[0]) for v in np.nonzero(nz & ~ok))
        raise PlanError('%s: corner %d of record %s (offset %d) leaves its window of %d rows' % (who, i, at, off[at], wrp))
      val = _window_read(x, rb, cb, np.where(nz, e - lo, 0), wrp, W)
      np.add.at(col, (k[nz], hh[nz], ww[nz]), wts[..., i][nz].astype(np.float64) * val[nz])

  if n0:
    small = tiles[n2 + n1:]
    _require(rec_off.size >= n0 * 2 * TW * KT * BW_TH and rec_w.size >= 4 * n0 * 2 * TW * KT * BW_TH, 'compact records: arrays too short')
    shape = (n0, 2, TW, KT, BW_TH)
    off = rec_off[:int(np.prod(shape))].reshape(shape)
    wts = rec_w[:4 * int(np.prod(shape))].reshape(shape + (4,))
    ti, hf, wc, k, px = np.indices(shape)
    hh, ww = small[ti, 0] + hf * BW_TH + px, small[ti, 1] + wc
    rb = (small[ti, 2] + hf * BW_TH) % H
    _require((wts[~((hh < H) & (ww < W))] == 0).all(), 'compact records: a pixel outside the image has a weight')
    run(off, wts, rb, small[ti, 3], BW_WR, 0, WC * BW_WR, hh, ww, k, 'weight gradient, compact tile')
    for h0, w0 in small[:, :2]:
      covered[h0:h0 + TH, w0:w0 + TW] += 1
  tall = np.zeros((H, W), dtype=bool)
  for h0, w0 in tiles[:n2 + n1, :2]:
    tall[h0:h0 + TH, w0:w0 + TW] = True
  want_rest = np.nonzero(tall.reshape(-1))[0]
  _require(nrest == want_rest.size and (_np(rest)[:nrest] == want_rest).all(),
           'the pixel list is not the sorted pixels of the tall-window tiles (%d listed, %d wanted)', nrest, want_rest.size)
  if polar is not None:
    pitems, prw, pro, n = _np(polar.items).astype(np.int64), _np(polar.rec_w), _np(polar.rec_off).astype(np.int64), polar.n
    _require(n > 0 and pitems.size == BP_ITEM_INTS * n and pro.size == KT * BW_TH * n and prw.size == 4 * KT * BW_TH * n, 'polar items: array sizes')
    pitems = pitems.reshape(n, BP_ITEM_INTS)
    _require((pitems[:, 0] % BW_TH == 0).all() and (pitems[:, 0] < H).all() and (pitems[:, 1] < W).all() and (pitems[:, :2] >= 0).all(),
             'polar items: an item outside the image or off the 32-row grid')
    _require((pitems[:, 2:2 + KT] >= 0).all() and (pitems[:, 2:2 + KT] < H).all() and (pitems[:, 2 + KT:] >= 0).all(),
             'polar items: a window base outside the image')
    shape = (n, KT, BW_TH)
    off, wts = pro.reshape(shape), prw.reshape(shape + (4,))
    it, k, px = np.indices(shape)
    hh, ww = pitems[it, 0] + px, pitems[it, 1]
    _require((wts[hh >= H] == 0).all(), 'polar records: a pixel outside the image has a weight')
    run(off, wts, pitems[it, 2 + k], pitems[it, 2 + KT + k], BP_WR, k * BP_TAPW, BP_TAPW, hh, ww, k, 'weight gradient, polar item')
    for h0, w in pitems[:, :2]:
      covered[h0:min(h0 + BW_TH, H), w] += 1
  else:
    np.add.at(covered.reshape(-1), _np(rest)[:nrest].astype(np.int64), 1)
  return col, covered, tall & (polar is None)


# ------------------------------------------------------------------------------------------------ adjoint plan
def check_adjplan(table, aplan, gcol):
  """(gx (H, W) float64 through the good tiles, good (H, W) bool) for gcol (9, H, W); structure of the adjoint plan."""
  H, W = gcol.shape[1:]
  _require(H % TH == 0 and W % TW == 0, 'an adjoint plan on a grid that is not whole tiles')
  good, ng, rec_off, rec_w, bad_ids, nbad, rec_off2, rec_w2 = aplan
  good = _np(good).astype(np.int64).reshape(-1, 4)
  _require(ng > 0 and good.shape[0] == ng, 'adjoint plan: %d good tiles listed, %d counted', good.shape[0], ng)
  six = good[:, 3] >> 16
  _require(((six == 0) | (six == 1)).all(), 'adjoint plan: flag bits other than the six-source flag')
  cbase = good[:, 3] & 0xffff
  _require((good[:, 0] % TH == 0).all() and (good[:, 1] % TW == 0).all() and (good[:, 0] >= 0).all() and (good[:, 0] < H).all() and
           (good[:, 1] >= 0).all() and (good[:, 1] < W).all() and (good[:, 2] >= 0).all() and (good[:, 2] < H).all(),
           'adjoint plan: a tile origin off the grid or a window base outside the image')
  cover = np.zeros((W, H), dtype=np.int64)  # (plane-transposed storage: the 64-pixel runs of the bad ids live there)
  for h0, w0 in good[:, :2]:
    cover[w0:w0 + TW, h0:h0 + TH] += 1
  ids = _np(bad_ids).astype(np.int64)[:nbad] if nbad else np.zeros(0, dtype=np.int64)
  _require((ids >= 0).all() and (ids < H * W // 64).all(), 'adjoint plan: a bad run id outside the image')
  np.add.at(cover.reshape(-1, 64), ids, 1)
  _require((cover == 1).all(), 'adjoint plan: good tiles + bad runs cover %d pixels not exactly once', int((cover != 1).sum()))
  goodmap = np.zeros((H, W), dtype=bool)
  # list lengths from the table alone
  nent = adjoint_list_lengths(table)
  for i, (h0, w0) in enumerate(good[:, :2]):
    goodmap[h0:h0 + TH, w0:w0 + TW] = True
    longest = int(nent[:, h0:h0 + TH, w0:w0 + TW].max())
    _require(longest <= 6, 'adjoint plan: good tile (%d, %d) has a list of %d entries', h0, w0, longest)
    _require((longest > 4) == bool(six[i]), 'adjoint plan: tile (%d, %d) has lists of up to %d entries and six flag %d', h0, w0, longest, six[i])
  shape = (ng, KT, AJ_PIX)
  o4, w4 = _np(rec_off).astype(np.int64).reshape(shape + (4,)), _np(rec_w).reshape(shape + (4,))
  o2, w2 = _np(rec_off2).astype(np.int64).reshape(shape + (2,)), _np(rec_w2).reshape(shape + (2,))
  ti, k, pix = np.indices(shape)
  wave = pix >> 5
  qh, qw = good[ti, 0] + (wave // TW) * 32 + (pix & 31), good[ti, 1] + wave % TW
  gx = np.zeros((H, W))
  nslots = np.zeros(shape, dtype=np.int64)
  for s in range(6):
    off, wts = (o4[..., s], w4[..., s]) if s < 4 else (o2[..., s - 4], w2[..., s - 4])
    nz = wts != 0
    if s >= 4:
      nz = nz & (six[ti] == 1)  # (the four-source instantiation never reads slots 4 and 5)
    colw, row = off // WR_SMALL, off % WR_SMALL
    ok = (off >= 0) & (colw < WC) & (cbase[ti] + colw < W)
    if (nz & ~ok).any():
      at = tuple(int(v[0]) for v in np.nonzero(nz & ~ok))
      raise PlanError('adjoint plan: slot %d of record %s (offset %d) is outside the 81 x 8 window or the image' % (s, at, off[at]))
    ph, pw = (good[ti, 2] + row) % H, np.minimum(cbase[ti] + colw, W - 1)
    np.add.at(gx, (qh[nz], qw[nz]), wts[nz].astype(np.float64) * gcol[k[nz], ph[nz], pw[nz]])
    nslots += nz
  _require((nslots == nent[k, qh, qw]).all(), 'adjoint plan: %d records do not have one live slot per list entry',
           int((nslots != nent[k, qh, qw]).sum()))
  return gx, goodmap


# ------------------------------------------------------------------------------------------------ the whole check
def check_plan(table, plan, aplan=None, seed=0):
  """Structure and values of `plan` (HF.sphere_plan, not None) and `aplan` (HF.sphere_adjplan or None) for `table`.  Returns the
  measured figures: {'sample': (error, bound), 'adjoint': (error / bound ratio, largest error) or None}."""
  table = table.detach().cpu().to(torch.float32)
  _require(table.dim() == 4 and table.shape[0] == 1 and table.shape[1] == 2 * KT, 'a table of %s', tuple(table.shape))
  H, W = table.shape[2:]
  rng = np.random.RandomState(seed)
  x = rng.standard_normal((H, W))
  want = sphere_conv_ref.im2col(torch.from_numpy(x).view(1, 1, H, W), table, 3, 3, 1, 1, H, W)[0, 0].numpy()
  bound = EPS * np.abs(x).max()
  fwd = sample_forward(table, plan, x)
  err = float(np.abs(fwd - want).max())
  _require(err <= bound, 'forward sampling through the plan: error %.3e beyond %.3e at %s', err, bound,
           np.unravel_index(np.abs(fwd - want).argmax(), want.shape))
  col, covered, listed = sample_records(table, plan, x)
  _require((covered == 1).all(), 'records: %d pixels are not covered exactly once', int((covered != 1).sum()))
  diff = np.where(listed[None], 0.0, np.abs(col - want))  # (pixels of the list are sampled by the general kernel, not through the plan)
  err = max(err, float(diff.max()))
  _require(diff.max() <= bound, 'record sampling through the plan: error %.3e beyond %.3e at %s', diff.max(), bound,
           np.unravel_index(diff.argmax(), diff.shape))
  out = {'sample': (err, float(bound)), 'adjoint': None}
  if aplan is not None:
    gcol = rng.standard_normal((KT, H, W))
    g = torch.from_numpy(gcol).view(1, 1, KT, H, W)
    want_gx = sphere_conv_ref.col2im_scatter(g, table, H, W, 3, 3, 1, 1)[0, 0].numpy()
    bound_gx = EPS * sphere_conv_ref.col2im_scatter(g.abs(), table, H, W, 3, 3, 1, 1)[0, 0].numpy() + 1e-12
    gx, goodmap = check_adjplan(table, aplan, gcol)
    d = np.where(goodmap, np.abs(gx - want_gx), 0.0)
    _require((d <= bound_gx).all(), 'adjoint through the plan: error %.3e at %s beyond its bound %.3e', d.max(),
             np.unravel_index(d.argmax(), d.shape), bound_gx[np.unravel_index(d.argmax(), d.shape)])
    out['adjoint'] = (float((d / bound_gx).max()), float(d.max()))
  return out
