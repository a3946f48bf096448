"""CPU tier of the fp16 spherical training entries (tests/split_ref.py, SPHERE_F16_CASES; GPU tier: tests/test_gpu_sphere_f16_precision.py;
DESIGN 3w6).  The planners are host code, so nothing here needs a GPU.

The headroom invariant.  The fp16 input gradient splits sx G_k[o][q], G_k the adjoint-sampled gradient and max |gy| sx < 2^15: it is a
finite fp16 number for any gy only while the weights of the list L(k, q) sum to <= 65504 / 2^15.  Asserted on the records the real
planner returns, for every table of the suite, the network's (128 x 256), 192 x 96, and two tables that cannot be safe.  Largest sums
(float64, from the table alone; stored column 1, taps 0 and 2 everywhere): 16 x 32 2.188, 32 x 64 2.176, 33 x 66 2.176, 64 x 128 2.173,
128 x 256 2.172 -- but only the 32 x 64 table had such a list inside a GOOD tile (its 64 rows wrap around, so every tile fits an 81-row
window): 2.176 in tile (0, 0), now a bad tile of the fp16 form's plan (fp32 gather kernel; the three-piece bf16 form keeps it).  Inside the good tiles the largest sums are
1.589 (32 x 64), 1.009 (128 x 256) and 1.024 (192 x 96); the plans of the last two are what they were.

Per case and role, as tests/test_split_ref_host.py does for the other families: the faithful emulation with an fp32 accumulator in the
kernel's summation order (chunk > tap > channel for the forward and the adjoint; the pixels of a tile, then the tiles, for the weight
gradient) stays under T / 1.5; every mutant is >= 3 T in the measure that judges it; the same mutant confined to ONE region (the
tall-window tiles of the forward, the six-slot tiles of the adjoint, one channel slice of a weight gradient) and one structural fault
per role (a lost channel chunk in one tile class, the polar items left out, a bad tile left unwritten) exceed T.  The scale mutant is
judged where tests/split_ref.py judges it everywhere: six-decades data with at least 21 columns, sized by its worst slice."""
import pytest
import torch

import sphere_plan_ref as PR
import sphere_tables as T
import split_ref as S
from mode_hip import functional as HF

HEADROOM = S.ADJ_F16_HEADROOM


def _record_sums(aplan):
  """(good tiles, 9, 256) float64: the sum of the weight magnitudes of all six slots of every record."""
  ng = aplan.ngood
  return aplan.rec_w.view(ng, 9, 256, 4).double().abs().sum(-1) + aplan.rec_w2.view(ng, 9, 256, 2).double().abs().sum(-1)


def _counts(aplan):
  six = (aplan.tiles.view(-1, 4)[:, 3] >> 16) & 1
  return aplan.ngood, int(six.sum()), aplan.nbad // 4


def _bad_tiles(aplan, H):
  """(h0, w0) of the bad tiles, from the 64-pixel run ids of the plane-transposed storage."""
  if aplan.bad_ids is None:
    return []
  px = aplan.bad_ids.to(torch.int64) * 64
  return sorted({(int(p % H), int(p // H) // 4 * 4) for p in px})


# name -> (table, (good, six-slot, bad) tiles of the adjoint plan or None, its bad tiles).  128 x 256 (the benchmark's and the
# conditioning probe's table) and 192 x 96 are the figures of the planner BEFORE it knew the headroom: they must not move.
POLES_128 = [(h0, w0) for h0 in (0, 64, 128, 192) for w0 in (0, 4, 120, 124)]
TABLES = {
    '16x32': (lambda: S.sphere_table(16, 32), None, None),
    '32x64': (lambda: S.sphere_table(32, 64), (7, 2, 1), [(0, 0)]),  # (before: (8, 3, 0) -- tile (0, 0) held the lists of 2.176)
    '33x66': (lambda: S.sphere_table(33, 66), None, None),
    '64x128': (lambda: S.sphere_table(64, 128), None, None),
    '128x256': (lambda: T.geometric(128, 256), (112, 8, 16), POLES_128),
    '192x96': (lambda: T.geometric(96, 192), (63, 6, 9), None),
}


@pytest.mark.parametrize('name', sorted(TABLES))
def test_every_adjoint_list_of_a_good_tile_is_inside_the_fp16_headroom(name):
  make, counts, bad = TABLES[name]
  pos = make()
  H, W = pos.shape[2:]
  sums = S.adjoint_weight_sums(pos)
  k, h, w = (int(v) for v in (sums == sums.max()).nonzero()[0])
  line = 'HEADROOM %-8s stored %3d x %3d | largest adjoint weight sum %.4f (tap %d, row %d, stored column %d)' % (name, H, W, float(sums.max()), k, h, w)
  aplan = HF.sphere_adjplan(pos, 3, 3, f16=True)
  if aplan is None:
    assert counts is None
    print(line + ' | no adjoint plan: every pixel on the fp32 gather kernel')
    return
  PR.check_plan(pos, HF.sphere_plan(pos, 3, 3), aplan)
  assert _counts(aplan) == counts
  if bad is not None:
    assert _bad_tiles(aplan, H) == sorted(bad)
  rs = _record_sums(aplan)
  ti, tap, pix = (int(v) for v in (rs == rs.max()).nonzero()[0])
  h0, w0 = aplan.tiles.view(-1, 4)[ti, :2].tolist()
  wave = pix >> 5
  print(line + ' | good %d (six-slot %d) bad %d | largest inside a good tile %.4f (tile (%d, %d), tap %d, pixel (%d, %d)) of %.4f allowed' %
        (counts + (float(rs.max()), h0, w0, tap, h0 + (wave // 4) * 32 + (pix & 31), w0 + wave % 4, HEADROOM)))
  assert float(rs.max()) <= HEADROOM
  # the three-piece bf16 form has no headroom to keep: its plan is the planner's of before, the heavy tiles still good
  full = HF.sphere_adjplan(pos, 3, 3, f16=False)
  PR.check_plan(pos, HF.sphere_plan(pos, 3, 3), full)
  assert _counts(full) == ((8, 3, 0) if name == '32x64' else counts)
  # the records and the table agree on what a list weighs (float32 weights against float64)
  good = S.sphere_f16_maps(pos).good
  assert abs(float(sums[:, good].max()) - float(rs.max())) < 1e-5
  assert not bool((good & (sums > HEADROOM).any(0)).any())


def test_tables_that_cannot_be_safe_lose_their_heavy_tiles():
  """The clustered table: six sources of weight 1 per list in its left half, inside one window -- good six-slot tiles for a planner that
  counts entries only.  They are bad tiles now; the right half (lists of one entry) stays good.  A contracted affine table never gets
  that far: a tile whose lists could weigh 2 spans more than 81 rows or 8 columns, and its only good tiles are those no tap reaches."""
  pos = T.clustered()
  sums = S.adjoint_weight_sums(pos)
  assert float(sums[:, :, :8].max()) == 6.0 and float(sums[:, :, 8:].max()) == 1.0
  assert int(PR.adjoint_list_lengths(pos).max()) == 6
  aplan = HF.sphere_adjplan(pos, 3, 3, f16=True)
  PR.check_plan(pos, HF.sphere_plan(pos, 3, 3), aplan)
  assert _counts(aplan) == (6, 0, 6) and sorted(set(aplan.tiles.view(-1, 4)[:, 1].tolist())) == [8, 12]
  assert float(_record_sums(aplan).max()) == 1.0
  print('HEADROOM clustered: largest sum 6.0 in the columns < 8: their 6 tiles are bad; 6 good tiles with sums of 1.0')
  pos = T.affine(1.0 / 3, 192, 16, 0.3, 0.3, 0.5)
  assert float(S.adjoint_weight_sums(pos).max()) > 2 * HEADROOM
  aplan = HF.sphere_adjplan(pos, 3, 3, f16=True)
  assert aplan is not None and float(_record_sums(aplan).max()) == 0.0  # (good tiles: the rows no tap reaches, every list empty)
  print('HEADROOM affine a = 1/3, b = 1/2: %d good tiles, none with a live list' % aplan.ngood)


def _plateau():
  case = next(c for c in S.SPHERE_F16_CASES if c.kind == S.PLATEAU)
  roles, t = S.sphere_f16_roles(case)
  return case, roles[0], t


def test_the_plateau_overflows_two_fp16_pieces_exactly_where_a_list_is_too_heavy():
  """The faithful two-piece emulation of the input gradient (pieces_f16 rounds through torch.float16 and overflows as v_cvt_pk_f16_f32
  does), evaluated on EVERY pixel whatever the plan says, is not finite on the plateau -- exactly at the pixels whose lists weigh more
  than the headroom in the plateau's direction -- and all of them are in tiles the planner keeps off the fp16 kernel; on the pixels that
  kernel still takes it is finite and within T / 1.5."""
  case, role, t = _plateau()
  pos, maps = t['pos'], t['maps']
  part = role.parts[0]
  assert part.name == 'fp16 tiles' and bool(maps.good.any())
  emu = part.emu[None]
  bad_px = ~torch.isfinite(emu).all(0).all(0)
  heavy = (S.adjoint_weight_sums(pos) > HEADROOM).any(0)
  sx = S.f16_scale_of(S.PLATEAU_C)
  over = (t['G'].double().abs() * sx >= 65520.0).any(0).any(0).any(0)  # (what rounds to infinity in fp16)
  print('PLATEAU %s: c sx = %.0f; %d pixels with a list above the headroom, %d where the scaled operand overflows, %d where the emulation is not finite, %d of them in good tiles' %
        (S.case_id(case), S.PLATEAU_C * sx, int(heavy.sum()), int(over.sum()), int(bad_px.sum()), int((bad_px & maps.good).sum())))
  assert S.PLATEAU_C * sx >= 2.0**15 * (1 - 2.0**-5)
  assert int(bad_px.sum()) > 0 and torch.equal(bad_px, over) and not bool((over & ~heavy).any())
  assert not bool((bad_px & maps.good).any()), 'the planner left a pixel that overflows on the fp16 kernel'
  whole, worst = S.part_measure(role, part, emu + role.noise())
  assert whole <= part.T / 1.5 and worst.rms <= part.T / 1.5, (whole, worst, part.T)


def _confine(part, m, where):
  return torch.where(where.expand_as(part.emu[None]), part.emu[m], part.emu[None])


def _one_region(role, part, m, maps):
  """(name, mask) of the ONE region a mutant is confined to."""
  like = part.emu[None]
  if role.chan_axis == 0:  # a weight gradient: the channels that make one slice, as tests/test_split_ref_host.py::_localised
    C = like.shape[0]
    n = min(C, -(-S.MIN_SLICE // (like.numel() // C)))
    mask = (torch.arange(C) < n).view(C, 1, 1, 1)
    return 'one slice of channels', mask
  if part.arith == 'bf16x6':
    return 'the fp32 tiles', part.mask
  if m[0] == 'scale':  # local by nature: the region that holds most of the judged columns next to the contract's edge
    edge = torch.zeros_like(part.mask)
    cols = int(part.mask.any(0).nonzero().max()) + 1
    edge[:, max(cols - 8, 0):cols] = True
    name = max(part.regions, key=lambda n: int((part.regions[n] & edge & part.mask).sum()))
    return name + ' (holds the contract edge)', part.regions[name]
  if role.name == 'forward':
    tall = maps.cls > 0
    return ('the tall-window tiles', tall) if bool(tall.any()) else ('the compact tiles (the table has no other)', maps.cls == 0)
  return 'the six-slot tiles', part.regions['six-slot tiles']


@pytest.mark.parametrize('case', S.SPHERE_F16_CASES, ids=S.case_id)
def test_faithful_passes_and_every_mutant_fails(case):
  roles, t = S.sphere_f16_roles(case)
  assert roles
  maps = t['maps']
  H, W = maps.cls.shape
  for role in roles:
    noise = role.noise()
    if role.name == 'forward':
      assert int((~maps.fwd_fp32).sum()) * 2 > H * W
    if role.name.startswith('weight gradient'):
      # The fp16 part is the larger one -- except at 33 x 66 (stored 66 x 33), where the planner's compact tiles are the seven ragged
      # 2-row tiles of the second tile row, 56 pixels of 2178, and the 64-row tiles above them are all of the mid class (polar items,
      # bf16 pieces).  The compact-only run there is a 56-pixel reduction; it is judged all the same.
      n_compact = int((maps.cls == 0).sum())
      assert (n_compact == 56) if case.shape[:2] == (33, 66) else (n_compact * 2 > H * W), (n_compact, H * W)
    for part in role.parts:
      tag = '%-62s %-32s %-12s' % (S.case_id(case), role.name, part.name)
      assert part.T > 0, tag
      n_el = part.emu[None].numel() if part.mask is None else int(part.mask.expand_as(part.emu[None]).sum())
      assert n_el >= S.MIN_SLICE, tag
      for name, rm in (part.regions or {}).items():
        assert int((rm & part.mask if part.mask is not None else rm).expand_as(part.emu[None]).sum()) >= S.MIN_SLICE, (tag, name)
      whole, worst = S.part_measure(role, part, part.emu[None] + noise)
      line = 'SPHEREF16HOST %s T %.3f | faithful + fp32: rms %.3f worst %.3f (/T %.2f; %s @ %s)' % (tag, part.T, whole, worst.rms, worst.rms / part.T, worst.axis, worst.index)
      assert whole <= part.T / 1.5 and worst.rms <= part.T / 1.5, line
      least = None
      for m in part.mutants:
        w_all = S.part_measure(role, part, part.emu[m])
        size = w_all[1].rms if m[0] == 'scale' else w_all[0]
        assert size >= 3 * part.T * (1 - 1e-12), (tag, m)
        where_name, where = _one_region(role, part, m, maps)
        w = S.part_measure(role, part, _confine(part, m, where))[1]
        line += ' | %s in %s: %.2f' % ('x'.join(str(v) for v in m), where_name, w.rms)
        assert w.rms > part.T, (tag, m, where_name, w, part.T)
        least = w.rms if least is None else min(least, w.rms)
      for name, (value, pname) in role.faults.items():
        if pname != part.name:
          continue
        w = S.part_measure(role, part, value)[1]
        line += ' | %s: %.3g' % (name, w.rms)
        assert w.rms > part.T, (tag, name, w, part.T)
        least = min(least, w.rms)
      print(line + ' | least mutant / T: %.2f' % (least / part.T))


def test_every_listed_table_role_and_kind_is_judged():
  """The grid the cases were chosen for, written out: forward and weight gradient at 16 x 32, 33 x 66 (groups 2, ragged tiles) and
  64 x 128, input gradient at 32 x 64 -- every kind of data, less the two spherical rules (no forward reads a gradient; the six-decades
  weight gradient up to 512 pixels) -- and the plateau on the input gradient."""
  got = set()
  for case in S.SPHERE_F16_CASES:
    for role in S.sphere_f16_roles(case)[0]:
      got.add((case.shape[:2], role.name.split(',')[0], case.kind))
  want = set()
  for table in ((16, 32), (33, 66), (64, 128)):
    for kind in S.KINDS:
      if kind != 'gradient-sized':
        want.add((table, 'forward', kind))
      if kind != 'six decades along a row' or table == (16, 32):
        want.add((table, 'weight gradient', kind))
  for kind in S.KINDS + (S.PLATEAU,):
    want.add(((32, 64), 'input gradient', kind))
  assert got == want, (sorted(got - want), sorted(want - got))
  assert HF.sphere_adjplan(S.sphere_table(64, 128), 3, 3, f16=True) is None  # (why the 64 x 128 table has no input gradient here)


# ------------------------------------------------------------------------------------------------ the explicit maxima change nothing
def _emulations_as_before(op, a, b, arith, mutants):
  """`emulations` as it stood before it took the maxima from outside, restated: the scales from the operands' own maxima."""
  def pieces(mutant):
    trunc = mutant == ('trunc',)
    if arith == 'bf16x6':
      return S.pieces_bf16(a, trunc), S.pieces_bf16(b, trunc), 1.0
    sa, sb = S.f16_scale_of(a.abs().max()), S.f16_scale_of(b.abs().max())
    if mutant is not None and mutant[0] == 'scale':
      sa = sa / 2.0**mutant[1]
    return S.pieces_f16(a, sa, trunc), S.pieces_f16(b, sb, trunc), sa * sb

  def emulate(mutant):
    pa, pb, s = pieces(mutant)
    pairs = [p for p in S.PAIRS[arith] if not (mutant is not None and mutant[0] == 'drop' and p == tuple(mutant[1:]))]
    out = None
    for i in sorted({p[0] for p in pairs}):
      term = op(pa[i - 1].double(), sum(pb[j - 1].double() for (ii, j) in pairs if ii == i))
      out = term if out is None else out + term
    return out / s

  out = {None: emulate(None)}
  pa, pb, s = pieces(None)
  for m in mutants:
    out[m] = out[None] - op(pa[m[1] - 1].double(), pb[m[2] - 1].double()) / s if m[0] == 'drop' else emulate(m)
  return out


SMALL = {('conv3d_s1', (2, 8, 8, 8, 8, 8)), ('conv3d_s1', (2, 16, 20, 5, 7, 33)), ('conv3d_s2', (3, 64, 128, 2, 4, 8)), ('deconv3d', (2, 64, 64, 3, 4, 8)),
         ('conv2d', (2, 16, 40, 7, 33, 1)), ('conv2d', (1, 64, 64, 12, 32, 2)), ('sphere', (16, 32, 1, 16, 32, 1)), ('sphere', (32, 64, 1, 64, 64, 1))}


@pytest.mark.parametrize('case', [c for c in S.CASES if (c.family, c.shape) in SMALL], ids=S.case_id)
def test_emulations_of_the_existing_cases_are_unchanged_bit_for_bit(case):
  """Every family, both arithmetics, every kind of data and every role, at the smaller shapes of CASES: `emulations` without maxima, and
  with the operands' own maxima handed in, gives the bits of the code it replaced."""
  for role in S.roles(case)[0]:
    muts = S.mutants_of(case, role)
    old = _emulations_as_before(role.op, role.a, role.b, case.arith, muts)
    for new in (S.emulations(role.op, role.a, role.b, case.arith, muts),
                S.emulations(role.op, role.a, role.b, case.arith, muts, (float(role.a.abs().max()), float(role.b.abs().max())))):
      assert set(new) == set(old)
      assert all(torch.equal(new[m], old[m]) for m in old), (S.case_id(case), role.name)
