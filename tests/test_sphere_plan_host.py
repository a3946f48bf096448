"""Host: the plans of the windowed spherical kernels (csrc/sphere_plan.hip, functional.sphere_plan / sphere_adjplan) on tables of any
size, checked by the numpy interpreter of tests/sphere_plan_ref.py -- the plan evaluated the way the kernels consume it, against the
float64 oracle, plus the structure the kernels rely on.  The planners run on the host, so nothing here needs a GPU.

Every case states the route its table takes and the class counts that make it non-vacuous (literals: what the planner yields today; a
planner that classifies differently has to explain itself here).  The synthetic tables of tests/sphere_tables.py reach what the
shift-invariant Cassini tables leave to a handful of tiles."""
import numpy as np
import pytest
import torch

import sphere_plan_ref as R
import sphere_tables as T
from mode_hip import functional as HF


def _plans(table):
  return HF.sphere_plan(table, 3, 3), HF.sphere_adjplan(table, 3, 3)


def _route(plan):
  """'usable': forward, weight gradient and the plane-transposed operators run on the plan; 'pixel list': a plan whose tall-window tiles
  have no polar items -- the NCHW weight gradient hands their pixels to the general kernel; 'forward only': no compact tile, only the
  forward runs on it; 'none': no plan, the general kernels."""
  if plan is None:
    return 'none'
  if HF._plan_usable(plan):
    return 'usable'
  return 'pixel list' if plan.counts[0] > 0 else 'forward only'


def _adjoint_counts(aplan):
  """(good tiles, six-source tiles among them, bad tiles) or None."""
  if aplan is None:
    return None
  six = (aplan.tiles.view(-1, 4)[:, 3] >> 16) & 1
  assert aplan.nbad % 4 == 0
  return aplan.ngood, int(six.sum()), aplan.nbad // 4


def _check(table, plan, aplan):
  out = R.check_plan(table, plan, aplan)
  print('table %s: sampling error %.3e (bound %.3e)%s' %
        (tuple(table.shape[2:]), out['sample'][0], out['sample'][1],
         '' if out['adjoint'] is None else ', adjoint error %.3e = %.3f of its bound' % (out['adjoint'][1], out['adjoint'][0])))
  return out


# (ih, iw) -> (compact, mid, wrap), polar items, (good, six-source, bad) adjoint tiles or None where H % 64 != 0
GEOMETRIC = {
    (36, 72): ((7, 11, 0), 80, None),
    (72, 144): ((48, 6, 0), 40, None),
    (81, 162): ((51, 4, 8), 78, None),
    (96, 192): ((63, 3, 6), 72, (63, 6, 9)),
    (100, 200): ((89, 3, 8), 80, None),
    (128, 256): ((112, 8, 8), 128, (112, 8, 16)),
    (160, 320): ((180, 10, 10), 160, (180, 10, 20)),
    (192, 384): ((258, 18, 12), 240, (259, 12, 29)),
    (256, 512): ((464, 32, 16), 384, (464, 16, 48)),
}


@pytest.mark.parametrize('ih,iw', sorted(GEOMETRIC))
def test_geometric_tables(ih, iw):
  """Cassini tables from 72 x 36 to 512 x 256: a usable plan with compact tiles and polar items, and -- where H is a multiple of 64 -- an
  adjoint plan with both tile classes and tiles left to the gather kernel."""
  table = T.geometric(ih, iw)
  assert tuple(table.shape[2:]) == (iw, ih)
  counts, npolar, adjoint = GEOMETRIC[(ih, iw)]
  plan, aplan = _plans(table)
  assert _route(plan) == 'usable'
  assert plan.counts == counts and plan.polar.n == npolar, (plan.counts, plan.polar.n)
  assert _adjoint_counts(aplan) == adjoint
  out = _check(table, plan, aplan)
  assert (out['adjoint'] is None) == (adjoint is None)


def test_a_cassini_table_is_shift_invariant_along_its_rows():
  """Why the synthetic tables exist: rolled by any number of rows, a Cassini table gives the same plan -- the same class counts."""
  base = T.geometric(96, 192)
  H = base.shape[2]
  for shift in (32, 64, 100):
    rolled = torch.roll(base, shift, 2).clone()
    rolled[0, 0::2] = torch.remainder(rolled[0, 0::2] + shift, H)
    plan, aplan = _plans(T._keep('rolled %d' % shift, lambda: rolled))
    assert plan.counts == GEOMETRIC[(96, 192)][0] and plan.polar.n == GEOMETRIC[(96, 192)][1]


def test_perturbed_table_takes_the_pixel_list_and_the_six_source_class():
  table = T.perturbed()
  plan, aplan = _plans(table)
  assert _route(plan) == 'pixel list'
  assert plan.counts == (51, 15, 6) and plan.polar is None and plan.nrest == 5376
  good, six, bad = _adjoint_counts(aplan)
  assert (good, six, bad) == (64, 56, 8) and six > good - six
  _check(table, plan, aplan)


# a -> route, (compact, mid, wrap), polar items or None, (good, six-source, bad) adjoint tiles
AFFINE = {
    0.5: ('forward only', (0, 12, 0), None, (4, 0, 8)),
    1.0: ('usable', (8, 4, 0), 32, (12, 0, 0)),
    1.5: ('pixel list', (4, 4, 4), None, (12, 0, 0)),
    2.5: ('pixel list', (4, 0, 8), None, (12, 0, 0)),
}


@pytest.mark.parametrize('a', sorted(AFFINE))
def test_affine_tables(a):
  """Row coordinate a h + dh + 0.3 on 192 x 16: mid and wrap tiles by the window heights whenever a != 1, coordinates in (-1, 0) and
  (H - 1, H), dead taps beyond the last row."""
  table = T.affine(a)
  rows = table[0, 0::2]
  cols = table[0, 1::2]
  assert int(((rows > -1) & (rows < 0)).sum()) > 0 and int(((cols > -1) & (cols < 0)).sum()) > 0  # the shifted-corner branch
  if a == 1.0:
    assert int(((rows > 191) & (rows < 192)).sum()) > 0
  route, counts, npolar, adjoint = AFFINE[a]
  plan, aplan = _plans(table)
  assert _route(plan) == route and plan.counts == counts
  assert (plan.polar.n if plan.polar is not None else None) == npolar
  assert _adjoint_counts(aplan) == adjoint
  _check(table, plan, aplan)


@pytest.mark.parametrize('a', [0.5, 1.0])
def test_halves_fit_demotes_tiles_of_an_affine_table(a):
  """A tile whose taps span no more than 81 rows and is of the mid class all the same: its 32-row halves do not fit 49-row windows at
  rbase and rbase + 32 (a = 0.5: the second half starts 16 rows below the first, not 32; a = 1: the first row's shifted corner sets
  rbase one row below where the second half needs it)."""
  table = T.affine(a)
  plan, _ = _plans(table)
  rows = R.tile_rows(table)
  tiles = plan.tiles.view(-1, 4)[:sum(plan.counts)].tolist()
  demoted = [(h0, w0) for h0, w0, _, cw in tiles if cw >> 16 == 1 and 0 < rows[(h0, w0)] <= R.WR_SMALL]
  assert len(demoted) == (12 if a == 0.5 else 4), demoted


def test_dead_taps():
  """NaN, +-inf, exactly -1 and exactly H / W coordinates are dead taps for the planners as for the oracle; one tile loses the row that
  set its rbase and is demoted by halves_fit."""
  table = T.dead_taps()
  t = table[0]
  assert int(torch.isnan(t).sum()) > 0 and int(torch.isinf(t).sum()) > 0 and int((t == -1).sum()) > 0
  assert int((t[0::2] == t.shape[1]).sum()) > 0 and int((t[1::2] == t.shape[2]).sum()) > 0
  plan, aplan = _plans(table)
  assert _route(plan) == 'usable'
  assert plan.counts == (62, 4, 6) and plan.polar.n == 80
  assert _adjoint_counts(aplan) == (63, 6, 9)
  rows = R.tile_rows(table)
  tiles = plan.tiles.view(-1, 4)[:72].tolist()
  assert [(h0, w0) for h0, w0, _, cw in tiles if cw >> 16 == 1 and rows[(h0, w0)] <= R.WR_SMALL] == [(64, 8)]
  _check(table, plan, aplan)


def test_sixteen_source_table_has_bad_adjoint_tiles_only():
  """Scale 0.25 inside every tile: every tile has lists of 32 entries, so no tile is good and there is no adjoint plan; the forward plan
  (mid tiles: the halves do not fit) is consistent."""
  table = T.sixteen_source()
  H, W = table.shape[2:]
  n = R.adjoint_list_lengths(table)
  assert all(int(n[:, h0:h0 + 64, w0:w0 + 4].max()) == 32 for h0 in range(0, H, 64) for w0 in range(0, W, 4))
  plan, aplan = _plans(table)
  assert aplan is None
  assert _route(plan) == 'forward only' and plan.counts == (0, 8, 0)
  _check(table, plan, None)


def _first_H_beyond_the_lds():
  """The first H whose wrap-around window of H + 1 rows is beyond 160 KiB (csrc/sphere_win_geometry.h, restated): 8 channels of
  chan_pitch(H + 1) floats (8 columns of H + 1 rows, padded to 32 banks modulo 64) + H + 1 + 8 floats of slack."""
  def lds_bytes(wr):
    pitch = 8 * wr + ((32 - (8 * wr) % 64) + 64) % 64
    return (8 * pitch + wr + 8) * 4
  H = 1
  while lds_bytes(H + 1) <= 160 * 1024:
    H += 1
  assert lds_bytes(H) <= 160 * 1024 < lds_bytes(H + 1)
  return H


def test_both_sides_of_the_lds_limit_of_the_wrap_around_window():
  H = _first_H_beyond_the_lds()
  assert H == 628
  below, above = T.affine(2.5, H - 1, 4), T.affine(2.5, H, 4)
  plan, aplan = _plans(below)
  assert _route(plan) == 'pixel list' and plan.counts == (6, 0, 4) and aplan is None
  _check(below, plan, None)
  assert HF.sphere_plan(above, 3, 3) is None and _route(None) == 'none'


# ------------------------------------------------------------------------------------------------ the interpreter rejects a wrong plan
def _mutable(plan):
  """A copy of a plan record, of the same record type, with every tensor cloned (the polar items' too)."""
  def copy(v):
    if isinstance(v, torch.Tensor):
      return v.clone()
    return _mutable(v) if isinstance(v, HF.PolarItems) else v
  return type(plan)(*(copy(v) for v in plan))


@pytest.fixture(scope='module')
def real_plan():
  table = T.geometric(96, 192)
  plan, aplan = _plans(table)
  R.check_plan(table, plan, aplan)
  n0, n1, n2 = plan.counts
  assert n0 and n1 and n2 and plan.polar is not None and aplan is not None
  return table, plan, aplan


def _live_record(rec_w, start=0):
  w = rec_w.view(-1, 4)
  return start + int(torch.nonzero((w[start:] != 0).all(1))[0])


@pytest.mark.parametrize('what', ['rbase', 'record offset', 'weight', 'class bit', 'polar rbase', 'polar record offset', 'polar weight'])
def test_the_interpreter_rejects_a_changed_plan(real_plan, what):
  table, plan, aplan = real_plan
  bad = _mutable(plan)
  tiles, (n0, n1, n2) = bad.tiles.view(-1, 4), bad.counts
  first_compact = n2 + n1
  if what == 'rbase':
    tiles[first_compact + 5, 2] = (tiles[first_compact + 5, 2] + 1) % table.shape[2]
  elif what == 'record offset':
    bad.rec_off[_live_record(bad.rec_w, 4000)] += 1
  elif what == 'weight':
    bad.rec_w.view(-1, 4)[_live_record(bad.rec_w, 4000), 2] += 0.25
  elif what == 'class bit':
    tiles[first_compact + 5, 3] |= 1 << 16
  elif what == 'polar rbase':
    bad.polar.items.view(-1, 20)[3, 2 + 4] += 1
  elif what == 'polar record offset':
    bad.polar.rec_off[_live_record(bad.polar.rec_w, 500)] += 1
  elif what == 'polar weight':
    bad.polar.rec_w.view(-1, 4)[_live_record(bad.polar.rec_w, 500), 1] += 0.25
  with pytest.raises(R.PlanError):
    R.check_plan(table, bad, aplan)
  R.check_plan(table, plan, aplan)  # (and the plan it was copied from is untouched)


@pytest.mark.parametrize('what', ['rbase', 'record offset', 'weight', 'six flag', 'bad run'])
def test_the_interpreter_rejects_a_changed_adjoint_plan(real_plan, what):
  table, plan, aplan = real_plan
  bad = _mutable(aplan)
  tiles = bad.tiles.view(-1, 4)
  if what == 'rbase':
    tiles[20, 2] = (tiles[20, 2] + 1) % table.shape[2]
  elif what == 'record offset':
    rec = _live_record(bad.rec_w, 9000)
    bad.rec_off[4 * rec + int(bad.rec_w.view(-1, 4)[rec].argmax())] += 1  # (the slot that carries the weight: a slot of 1e-6 stays within the bound)
  elif what == 'weight':
    bad.rec_w[4 * _live_record(bad.rec_w, 9000)] += 0.25
  elif what == 'six flag':
    assert tiles[0, 3] >> 16 == 1  # the six-source tiles come first
    tiles[0, 3] &= 0xffff
  elif what == 'bad run':
    bad.bad_ids[0] += 1
  with pytest.raises(R.PlanError):
    R.check_plan(table, plan, bad)
