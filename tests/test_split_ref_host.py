"""CPU tier: the emulation of tests/split_ref.py separates a faithful split-operand kernel from a subtly wrong one on every case the
GPU tier (tests/test_gpu_split_precision.py) runs, and the bounds the older tests use do not.

For every shared case and role, from the case's own inputs:
  * the faithful emulation plus the error of a plain fp32 evaluation (torch's CPU operator on the fp32 tensors; the oracle on fp32
    tensors for the sphere) has a worst slice <= T / 1.5: a kernel that keeps the contract and accumulates like an fp32 sum passes
    with room to spare;
  * every mutant is >= 3 T by construction of T;
  * the same mutant confined to one output channel (one slice of channels where a channel is smaller than a slice), or to the last
    partial column tile, has a worst slice > T: a fault in one place is seen although the whole-tensor figure barely moves.
Pieces and the scale are checked bit for bit against their definitions in csrc/split_arith.h.

The eval entries (tests/test_gpu_eval_precision.py) get the same three conditions for every case and epilogue variant, the three epilogue
mutants on top, and the factors by which the bounds of the older eval tests admit a lost product and a stale fold.

The training entries of the fp32 kernels (tests/test_gpu_grad32_precision.py) get the three conditions for every role of
GRAD32_CASES, the structural faults of those kernels on top (end of this file), and -- in
test_the_bounds_of_the_older_tests_admit_every_single_pair_mutant -- the factors by which the max-abs bounds of tests/test_gpu_kernels.py
admit each of those faults in a quiet block of channels."""
import numpy as np
import pytest
import torch

import split_ref as S


def _localised(case, role, ref, m, where):
  """The faithful value everywhere but in one output channel / the last partial column tile, where it is the mutant's.  Where a channel
  holds fewer than the 256 elements of a slice (the smallest outputs: 24 at 3 x 128 x 1 x 2 x 4), the fault takes the consecutive channels
  that make one slice -- the finest thing the metric resolves."""
  got = ref.emu[None].clone()
  bad = ref.emu[m]
  if where == 'channel':
    C = got.shape[role.chan_axis]
    g = min(C, -(-S.MIN_SLICE // (got.numel() // C)))
    got.narrow(role.chan_axis, 0, g).copy_(bad.narrow(role.chan_axis, 0, g))
  else:
    n = role.cols  # (the judged columns: a two-piece case on six-decades data ends before the row does)
    k = n % 32 or 8
    got.narrow(role.col_axis, n - k, k).copy_(bad.narrow(role.col_axis, n - k, k))
  return got


@pytest.mark.parametrize('case', S.CASES, ids=S.case_id)
def test_faithful_passes_and_every_mutant_fails(case):
  roles, _ = S.roles(case)
  assert roles
  for role in roles:
    ref = S.reference(case, role)
    tag = (S.case_id(case), role.name)
    assert ref.T > 0, tag
    plain = role.plain32().double()
    whole, worst, rest = S.measure(case, role, ref, ref.emu[None] + (plain - ref.want))
    line = '%-64s %-22s T %.3f | faithful + fp32: rms %.3f worst slice %.3f (axis %d @ %d)' % (tag + (ref.T, whole, worst.rms, worst.axis, worst.index))
    assert worst.rms <= ref.T / 1.5 and whole <= ref.T / 1.5, line
    for m in ref.mutants:
      size = S.mutant_size(case, role, m, ref.emu[m], ref.want, ref.den)
      assert size >= 3 * ref.T * (1 - 1e-12), (tag, m)
      if m[0] == 'scale':
        continue  # (local by nature, and sized by its worst slice: mutant_size)
      for where in ('channel', 'columns'):
        if where == 'columns' and role.col_axis is None:
          continue
        w = S.measure(case, role, ref, _localised(case, role, ref, m, where))[1]
        line += ' | %s in one %s: %.2f' % ('x'.join(str(v) for v in m), where, w.rms)
        assert w.rms > ref.T, (tag, m, where, w, ref.T)
    print(line + ('' if rest is None else ' | columns past the contract (not judged): rms %.2f' % rest))


def test_pieces_sum_to_the_value_bit_for_bit():
  r = np.random.RandomState(7)
  a = torch.from_numpy((r.standard_normal(200000) * np.exp(r.uniform(-30, 30, 200000))).astype(np.float32))
  a[:3] = torch.tensor([0.0, -0.0, 1.0])  # (magnitudes e^-30 .. e^30: every remainder a normal fp32 number, no piece rounds to infinity)
  p1, p2, p3 = S.pieces_bf16(a)
  for p in (p1, p2, p3):
    assert torch.equal(p, p.to(torch.bfloat16).float())  # each piece IS a bf16 value
  assert torch.equal(p1.double() + p2.double() + p3.double(), a.double())
  assert torch.equal((p1 + p2) + p3, a)
  # the third piece is the exact remainder: truncating it instead of rounding changes nothing (why that mutant enters no threshold)
  assert all(torch.equal(x, y) for x, y in zip(S.pieces_bf16(a, trunc_last=True), (p1, p2, p3)))
  # two fp16 pieces of the scaled value: the leading 22 bits, the remainder exact in fp32
  b = torch.from_numpy(r.standard_normal(200000).astype(np.float32))
  s = S.f16_scale_of(b.abs().max())
  h1, h2 = S.pieces_f16(b, s)
  big = b.abs() * s >= 2.0**-3  # (both pieces normal fp16 numbers)
  err = ((h1.double() + h2.double()) / s - b.double()).abs()
  assert bool((err[big] <= 2.0**-22 * b.double().abs()[big]).all())
  t1, t2 = S.pieces_f16(b, s, trunc_last=True)
  assert torch.equal(t1, h1) and bool((t2.abs() <= h2.abs()).all()) and not torch.equal(t2, h2)
  rem = (b * s - h1).double()
  assert bool(((rem - t2.double()).abs() <= (rem - h2.double()).abs() * 2 + 2.0**-24).all()) and bool((t2.double().abs() <= rem.abs()).all())


def test_f16_scale_of_as_its_comment_states_it():
  for m in (1.0, 1.5, 0.75, 3.9e4, 6.1e-5, 1e-7, 2.0**-60, 1e30):
    s = S.f16_scale_of(m)
    assert 2.0**14 <= m * s < 2.0**15 and s == 2.0**round(np.log2(s)), m
  assert S.f16_scale_of(0.0) == 1.0
  assert S.f16_scale_of(2.0**-70) == S.f16_scale_of(2.0**-63) == 2.0**77  # magnitudes below 2^-63 are treated as 2^-63
  assert np.isfinite(S.f16_scale_of(float('inf'))) and np.isfinite(S.f16_scale_of(float('nan')))


def test_emulate_with_every_pair_is_the_product_of_the_kept_bits():
  """Six bf16 pairs leave out a2 b3 + a3 b2 + a3 b3 <= 3 * 2^-24 |a||b|; three fp16 pairs a2 b2 <= 2^-22 |a||b|: the faithful emulation
  is within that of the float64 operator, componentwise; and `emulations` (a dropped pair as one subtraction) agrees with `emulate`."""
  case = next(c for c in S.CASES if c.family == 'conv3d_s1' and c.shape == (2, 8, 8, 8, 8, 8) and c.kind == 'unit variance')
  for arith in ('bf16x6', 'f16x3'):
    role = S.roles(case._replace(arith=arith))[0][0]
    want = role.op(role.a.double(), role.b.double())
    den = role.op(role.a.double().abs(), role.b.double().abs())
    u = S.units(S.emulate(role.op, role.a, role.b, arith), want, den, arith)
    assert float(u.max()) <= (3.0 if arith == 'bf16x6' else 1.0)
    both = S.emulations(role.op, role.a, role.b, arith, S.DROPS[arith])
    for m in S.DROPS[arith]:
      direct = S.emulate(role.op, role.a, role.b, arith, m)
      assert float(((both[m] - direct).abs() / den).max()) <= 2.0**-45, m
    # the truncation mutant: the identity on three bf16 pieces, within twice the faithful error on two fp16 pieces -- it enters no T
    faithful, trunc = both[None], S.emulate(role.op, role.a, role.b, arith, ('trunc',))
    if arith == 'bf16x6':
      assert torch.equal(trunc, faithful)
    else:
      r_f, r_t = S.rms(S.units(faithful, want, den, arith)), S.rms(S.units(trunc, want, den, arith))
      print('fp16 pieces, last piece truncated: rms %.3f against %.3f faithful' % (r_t, r_f))
      assert not torch.equal(trunc, faithful) and r_t <= 2 * r_f


def test_worst_slice_groups_short_axes_and_skips_nothing():
  shape = (3, 5, 7, 11)  # elements per index: 385, 231, 165, 105 -> groups of 1, 2, 2, 3 indices; the short tails join the group before
  want_sizes = {0: 385, 1: 3 * 231, 2: 3 * 165, 3: 5 * 105}
  for ax in range(4):
    v = torch.zeros(shape, dtype=torch.float64)
    v.select(ax, shape[ax] - 1).fill_(1.0)  # the last index of the axis: in a tail group
    got = S.worst_slice(v)
    # the slice along `ax` that holds the ones is the worst: the fraction of ones in it is the last index's share of its group
    share = (v.numel() // shape[ax]) / float(want_sizes[ax])
    assert got.axis == ax and abs(got.rms - share**0.5) < 1e-12, (ax, got, share)
  with pytest.raises(AssertionError):
    S.units(torch.ones(4), torch.zeros(4), torch.tensor([1.0, 0.0, 1.0, 1.0]), 'bf16x6')  # non-zero where every product is zero


# ------------------------------------------------------------------------------------------------ why this file exists
def _old_bounds_admit(case, role_name, bound_of):
  role = next(r for r in S.roles(case)[0] if r.name == role_name)
  ref = S.reference(case, role)
  plain = role.plain32().double()
  bound = bound_of(role, ref.want)
  out = []
  for m in [None] + list(ref.mutants):
    got = ref.emu[m] + (plain - ref.want)  # the arithmetic (or a mutant of it) plus an fp32 accumulator's rounding
    e = float((got - ref.want).abs().max())
    out.append((m, e, bound, S.measure(case, role, ref, got)[0], ref.T))
  return out


def test_the_bounds_of_the_older_tests_admit_every_single_pair_mutant():
  """tests/test_gpu_split.py holds a forward to 2^-22 sqrt(terms) 8 max|y| and a weight gradient to 2e-5 max|gw|.  At 32 -> 32, 6 x 10 x 40
  a kernel that lost ANY one of a2 b2, a1 b3, a3 b1 stays below both by a wide margin -- and exceeds T by the factor of three T is made of."""
  case = next(c for c in S.CASES if c.family == 'conv3d_s1' and c.shape == (1, 32, 32, 6, 10, 40) and c.kind == 'unit variance' and c.arith == 'bf16x6')
  fwd = _old_bounds_admit(case, 'forward', lambda role, want: 2.0**-22 * np.sqrt(32 * 27) * 8 * max(1.0, float(want.abs().max())))
  wgr = _old_bounds_admit(case, 'weight gradient', lambda role, want: 2e-5 * max(1.0, float(want.abs().max())))
  for name, rows in (('forward', fwd), ('weight gradient', wgr)):
    for m, e, bound, whole, T in rows:
      print('%-16s %-14s max error %.2e, old bound %.2e (x %.0f) | componentwise rms %.2f, T %.2f' % (name, m, e, bound, bound / e, whole, T))
      assert e <= bound / 4, (name, m)  # admitted, faithful and mutant alike
      assert (whole <= T / 1.5) if m is None else (whole >= 2.5 * T), (name, m, whole, T)
  # The fp32 training entries: tests/test_gpu_kernels.py holds an output or an input gradient to 2e-6 (reduction terms)
  # max(1, max|ref|) and a weight gradient to 2e-5 max(1, max|gw|), relative to the tensor's LARGEST element.  One line per family and
  # structural fault (S.structural_faults, on the family's first unit-variance case): the factor by which that bound admits the fault
  # when the output channels it sits in are quiet -- scaled by 2^-20, a power of two: want, den and the fault scale exactly, so the
  # componentwise figure is the one the host tier asserts to exceed T, unchanged.  The fp32 accumulator's own error rides along at full size.
  quiet = 2.0**-20
  for fam in ('conv3d_s1', 'conv3d_s2', 'deconv3d', 'conv3d_c1', 'conv2d', 'conv2d_s2', 'conv1x1', 'conv_stem'):
    case = next(c for c in S.GRAD32_CASES if c.family == fam and c.kind == 'unit variance' and c.route == 'f32')
    lines = 0
    for role, ref in S.grad32_references(case, S.grad32_roles(case)[0]):
      if role.acc is not None:
        continue
      noise = float((role.plain32().double() - ref.want).abs().max())
      C = ref.want.shape[role.chan_axis]
      terms = role.b.numel() // role.b.shape[0 if role.name == 'forward' and fam != 'deconv3d' else 1]
      if fam == 'deconv3d':
        terms = 27 * role.a.shape[1]
      for name, (value, n) in S.structural_faults(case, role, ref).items():
        if n is not None and n >= C:
          continue  # (the block is the whole tensor: nothing louder beside it)
        loud = ref.want.narrow(role.chan_axis, n, C - n) if n is not None else ref.want
        bound = (2e-5 if role.name == 'weight gradient' else 2e-6 * terms) * max(1.0, float(loud.abs().max()))
        e = float((value - ref.emu[None]).abs().max()) * quiet + noise
        worst = S.measure(case, role, ref, value)[1].rms
        print('%-10s %-16s %-20s in a block 2^-20 of the rest: max error %.2e, old bound %.2e (x %.0f) | componentwise worst slice %.3g, T %.2f' %
              (fam, role.name, name, e, bound, bound / e, worst, ref.T))
        assert bound / e > 1 and worst > ref.T, (fam, role.name, name)
        lines += 1
    assert lines, fam


# ------------------------------------------------------------------------------------------------ the eval entries
def _localised_eval(case, role, ref, m, where):
  """_localised, the channel fault in the slice of channels ReLU leaves most alive (the largest share of non-zero `want`): a channel whose
  outputs ReLU has set to zero shows no fault because there is none left to show (a typical shift or non-negative data under weights that
  sum below zero silences most of a channel: measured 0.34 against T 0.57 in such a one, stride 2, 32 -> 64)."""
  if where != 'channel':
    return _localised(case, role, ref, m, where)
  got = ref.emu[None].clone()
  C = got.shape[1]
  g = min(C, -(-S.MIN_SLICE // (got.numel() // C)))
  alive = (ref.want != 0).double().mean([d for d in range(got.dim()) if d != 1])
  c0 = max(range(0, C - g + 1, g), key=lambda c: float(alive[c:c + g].mean()))
  got.narrow(1, c0, g).copy_(ref.emu[m].narrow(1, c0, g))
  return got


@pytest.mark.parametrize('case', S.EVAL_CASES, ids=S.eval_case_id)
def test_eval_faithful_passes_and_every_mutant_fails(case):
  """The conditions of test_faithful_passes_and_every_mutant_fails for every eval case and every epilogue variant the GPU tier
  (tests/test_gpu_eval_precision.py) runs -- the plain evaluation is torch's CPU fp32 operator on x and the folded weights w' plus the
  fp32 epilogue -- and: each epilogue mutant (one channel's fold scale off by 2^-12, a shift taken from the neighbouring channel, the
  residual of output block 1 read from block 0 in the last column tile) exceeds T in its worst slice."""
  lin = S.eval_linear(case)
  role = lin.role
  for relu, with_add in case.epilogues:
    ref = S.eval_reference(case, lin, relu, with_add)
    tag = (S.eval_case_id(case), 'relu %d add %d' % (relu, with_add))
    assert ref.T > 0, tag
    whole, worst, rest = S.measure(case, role, ref, ref.emu[None] + S.eval_accumulation(case, lin, relu, with_add))
    line = '%-72s %-14s T %.3f | faithful + fp32: rms %.3f worst slice %.3f (axis %d @ %d)' % (tag + (ref.T, whole, worst.rms, worst.axis, worst.index))
    assert worst.rms <= ref.T / 1.5 and whole <= ref.T / 1.5, line
    for m in ref.mutants:
      size = S.mutant_size(case, role, m, ref.emu[m], ref.want, ref.den)
      assert size >= 3 * ref.T * (1 - 1e-12), (tag, m)
      if m[0] == 'scale':
        continue
      for where in ('channel', 'columns'):
        w = S.measure(case, role, ref, _localised_eval(case, role, ref, m, where))[1]
        line += ' | %s in one %s: %.2f' % ('x'.join(str(v) for v in m), where, w.rms)
        assert w.rms > ref.T, (tag, m, where, w, ref.T)
    for name, value in S.epilogue_mutants(case, lin, relu, with_add).items():
      w = S.measure(case, role, ref, value)[1]
      line += ' | %s: %.2f' % (name, w.rms)
      assert w.rms > ref.T, (tag, name, w, ref.T)
    print(line + ('' if rest is None else ' | columns past the contract (not judged): rms %.2f' % rest))


# (Three bf16 pieces only.  On two fp16 pieces and unit-variance data a lost product is 2^-11 of a term and T, a third of it, is 12 - 20 units
# of 2^-22: a stale fold of 1e-5 -- 2 units there -- is inside T, and both old bounds see the lost product.  What holds the fold of the fp16
# entries is the 2^-12 epilogue mutant, 40 - 130 units in every such case, the six-decades kind whose T is 0.2 - 0.3, and the kept-pack
# check of the GPU tier.)
OLD_EVAL_BOUNDS = [('conv3d_s1', (1, 32, 32, 6, 10, 40), 'bf16x6'), ('conv2d', (1, 64, 64, 12, 32, 2), 'bf16x6'), ('deconv3d', (2, 64, 32, 4, 6, 16), 'bf16x6')]


@pytest.mark.parametrize('fam,shape,arith', OLD_EVAL_BOUNDS)
def test_the_bounds_of_the_older_eval_tests_admit_the_mutants(fam, shape, arith):
  """tests/test_gpu_kernels.py::test_folded_batchnorm_* hold an eval entry to an absolute 1e-4, tests/test_gpu_f16.py::test_eval_epilogues_*
  to 2^-22 sqrt(terms) max|y|.  On the inputs of the unit-variance, typical-BatchNorm cases a three-piece kernel that lost the mildest
  partial product stays below both, and one whose fold of ONE channel is stale by a relative 1e-5 (~170 units of 2^-24 of that channel's
  convolution) stays below the 1e-4 -- by the factors printed -- while both exceed T.  (The 2^-22 sqrt(terms) max|y| bound is NOT
  asserted to admit the stale fold: 1e-5 of a channel's largest output against 7e-6 .. 1.4e-5 of the tensor's is a coin's toss; its factor
  is printed.  The 2^-12 of the epilogue mutants is what every case must catch, and neither old bound admits that one everywhere.)"""
  case = next(c for c in S.EVAL_CASES if (c.family, c.shape, c.arith, c.bn, c.route) == (fam, shape, arith, 'typical', 'split' if arith == 'bf16x6' else 'f16'))
  lin = S.eval_linear(case)
  role = lin.role
  terms = role.b[0].numel() if lin.waxis == 0 else role.b.shape[0] * 27
  for relu, with_add in case.epilogues:
    ref = S.eval_reference(case, lin, relu, with_add)
    acc = S.eval_accumulation(case, lin, relu, with_add)  # an fp32 accumulator's rounding
    bounds = {'1e-4': 1e-4, '2^-22 sqrt(terms) max': 2.0**-22 * np.sqrt(terms) * float(ref.want.abs().max())}
    mild = min(ref.mutants, key=lambda m: S.mutant_size(case, role, m, ref.emu[m], ref.want, ref.den))
    stale = lin.emu_lin[None].clone()
    stale[:, stale.shape[1] // 2] *= 1.0 + 1e-5
    stale = S.epilogue64(stale, lin.beta.double() - lin.mean.double() * lin.s32.double(), lin.add if with_add else None, relu)
    for name, value in (('faithful', ref.emu[None]), ('x'.join(str(v) for v in mild), ref.emu[mild]), ('stale fold 1e-5', stale)):
      got = value + acc
      e = float((got - ref.want).abs().max())
      whole, worst, _ = S.measure(case, role, ref, got)
      print('%-44s relu %d add %d %-16s max error %.2e | 1e-4: x %.0f | 2^-22 sqrt(%d) max = %.2e: x %.1f | rms %.2f worst slice %.2f, T %.2f' %
            (S.eval_case_id(case), relu, with_add, name, e, 1e-4 / e, terms, bounds['2^-22 sqrt(terms) max'], bounds['2^-22 sqrt(terms) max'] / e,
             whole, worst.rms, ref.T))
      if name == 'faithful':
        assert worst.rms <= ref.T / 1.5 and e < 1e-4
      else:
        assert worst.rms > ref.T, (name, worst, ref.T)
        if name == 'stale fold 1e-5' or arith == 'bf16x6':  # (a lost product of TWO fp16 pieces is 2^-11 of a term: both old bounds see that)
          assert e < 1e-4, (name, e)  # admitted by the absolute bound
        if name != 'stale fold 1e-5' and arith == 'bf16x6':
          assert e <= bounds['2^-22 sqrt(terms) max'], (name, e)


# ------------------------------------------------------------------------------------------------ the fp32 gradient entries
def _worst_in(case, role, ref, value):
  return S.measure(case, role, ref, value)[1]


@pytest.mark.parametrize('case', S.GRAD32_CASES, ids=S.grad32_case_id)
def test_grad32_faithful_passes_and_every_mutant_fails(case):
  """The three conditions of test_faithful_passes_and_every_mutant_fails for every role of every case tests/test_gpu_grad32_precision.py
  runs on the fp32 kernels (judged under the three-piece T of the same inputs), and: each structural fault these kernels can commit
  (S.structural_faults: a reduction tail that meets zero, a lost K-slice, a lost last pixel segment, a dropped tap -- all confined to one
  block of output channels) has a worst slice > T."""
  roles, _ = S.grad32_roles(case)
  assert roles
  for role, ref in S.grad32_references(case, roles):
    tag = (S.grad32_case_id(case), role.name)
    assert ref.T > 0, tag
    plain = role.plain32().double()
    whole, worst, _ = S.measure(case, role, ref, ref.emu[None] + (plain - ref.want))
    line = 'GRAD32HOST %-58s %-22s T %.3f | faithful + fp32: rms %.3f worst slice %.3f (/T %.2f; axis %d @ %d)' % (
        tag + (ref.T, whole, worst.rms, worst.rms / ref.T, worst.axis, worst.index))
    assert worst.rms <= ref.T / 1.5 and whole <= ref.T / 1.5, line
    for m in ref.mutants:
      assert S.mutant_size(case, role, m, ref.emu[m], ref.want, ref.den) >= 3 * ref.T * (1 - 1e-12), (tag, m)
      for where in ('channel', 'columns'):
        if where == 'columns' and (role.col_axis is None or not S.column_fault_resolvable(role, ref.want)):
          continue
        w = _worst_in(case, role, ref, _localised(case, role, ref, m, where))
        line += ' | %s in one %s: %.2f' % ('x'.join(str(v) for v in m), where, w.rms)
        assert w.rms > ref.T, (tag, m, where, w, ref.T)
    for name, (value, _) in S.structural_faults(case, role, ref).items():
      w = _worst_in(case, role, ref, value)
      line += ' | %s: %.3g' % (name, w.rms)
      assert w.rms > ref.T, (tag, name, w, ref.T)
    print(line)
