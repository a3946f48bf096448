"""CPU tier of the BatchNorm contract (tests/bn_ref.py, tests/test_gpu_batchnorm_forms.py): the float64 reference is nn.BatchNorm's
definition, the generators deliver what they promise for every case of the GPU tier, and the exact checks of the GPU tier can see the
damage they exist for (a 16-byte piece lost or taken twice by a statistics loop)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import bn_ref as R

SMALL = [((2, 3, 7), 1), ((4, 6, 1028), 2), ((6, 2, 515), 3), ((1, 2, 1031), 1)]


def _module(C, dims, momentum=0.1, track=True):
  bn = (nn.BatchNorm3d if dims == 5 else nn.BatchNorm2d)(C, momentum=momentum, track_running_stats=track).double()
  g = torch.Generator().manual_seed(7)
  with torch.no_grad():
    bn.weight.copy_(1 + 0.2 * torch.randn(C, generator=g))
    bn.bias.copy_(0.3 * torch.randn(C, generator=g))
  return bn


@pytest.mark.parametrize('relu,with_add', [(False, False), (True, False), (True, True), (False, True)])
@pytest.mark.parametrize('shape,groups', SMALL)
def test_reference_is_the_module_in_float64(shape, groups, relu, with_add):
  """Forward and backward; a statistics group is one call of the module (running statistics included, here kept in float64)."""
  B, C, S = shape
  c = R.random_case(shape, groups)
  bn = _module(C, 4)
  y = c['y'].double().requires_grad_(True)
  add = c['add'].double().requires_grad_(True)
  o = torch.cat([bn(p.reshape(-1, C, S, 1)).reshape(-1, C, S) for p in y.chunk(groups, 0)], 0)
  o = o + add if with_add else o
  o = torch.relu(o) if relu else o
  o.backward(c['gout'].double())
  case = dict(c, gamma=bn.weight.detach(), beta=bn.bias.detach())
  ref = R.reference(case, relu, with_add, groups)
  scale = lambda t: max(1.0, float(t.abs().max()))
  assert float((ref['out'] - o.detach()).abs().max()) <= 1e-12
  assert float((ref['gy'] - y.grad).abs().max()) <= 1e-12 * scale(y.grad)
  assert float((ref['ggamma'] - bn.weight.grad).abs().max()) <= 1e-12 * scale(bn.weight.grad)
  assert float((ref['gbeta'] - bn.bias.grad).abs().max()) <= 1e-12 * scale(bn.bias.grad)
  if with_add:
    assert float((ref['gadd'] - add.grad).abs().max()) <= 1e-12
  assert int(bn.num_batches_tracked) == groups


@pytest.mark.parametrize('momentum', [0.1, 1.0, None])
def test_running_statistics_over_three_calls(momentum):
  """Three consecutive calls (momentum=None: the cumulative average, momentum 1 / n at the n-th call); the reference rounds every update
  to float32, the float64 module does not: equal to float32 round-off, and to 1e-12 when the module's state is rounded the same way."""
  shape = (4, 3, 130)
  bn = _module(3, 5, momentum)
  rm, rv = torch.zeros(3), torch.ones(3)
  for call in range(3):
    c = R.random_case(shape, 1, seed=90 + call)
    fwd = R.forward(c['y'], bn.weight.detach(), bn.bias.detach())
    with torch.no_grad():
      o = bn(c['y'].double().reshape(4, 3, 130, 1, 1)).reshape(shape)
      m = momentum if momentum is not None else 1.0 / (call + 1)
      rm, rv = R.running_update(fwd, rm, rv, m)
      assert float((rm.double() - bn.running_mean).abs().max()) <= 2.0**-24 * float(bn.running_mean.abs().max()) + 1e-12
      assert float((rv.double() - bn.running_var).abs().max()) <= 2.0**-24 * float(bn.running_var.abs().max()) + 1e-12
      bn.running_mean.copy_(rm)
      bn.running_var.copy_(rv)
    assert float((fwd['out'] - o).abs().max()) <= 1e-12
  assert int(bn.num_batches_tracked) == 3


def test_groups_update_the_running_statistics_like_consecutive_calls():
  shape, groups = (6, 2, 515), 3
  c = R.random_case(shape, groups)
  bn = _module(2, 4)
  with torch.no_grad():
    for p in c['y'].double().chunk(groups, 0):
      bn(p.reshape(2, 2, 515, 1))
  fwd = R.forward(c['y'], bn.weight.detach(), bn.bias.detach(), groups=groups)
  rm, rv = R.running_update(fwd, torch.zeros(2), torch.ones(2), 0.1)
  assert float((rm.double() - bn.running_mean).abs().max()) <= 3 * 2.0**-24 * float(bn.running_mean.abs().max())
  assert float((rv.double() - bn.running_var).abs().max()) <= 3 * 2.0**-24 * float(bn.running_var.abs().max())


@pytest.mark.parametrize('training', [True, False])
def test_without_tracked_statistics_the_batch_statistics_are_used(training):
  shape = (2, 3, 130)
  c = R.random_case(shape, 1)
  bn = _module(3, 4, track=False).train(training)
  with torch.no_grad():
    o = bn(c['y'].double().reshape(2, 3, 130, 1)).reshape(shape)
  assert bn.running_mean is None
  assert float((R.forward(c['y'], bn.weight.detach(), bn.bias.detach())['out'] - o).abs().max()) <= 1e-12


def test_the_case_table_reaches_the_regimes_it_names():
  for shape, groups, _, _ in R.GRID_CASES:
    B, C, S = shape
    assert (R.pick_nsplit(C * groups, S), R.apply_chunks(B * C, S)) == R.GRID_GEOMETRY[(shape, groups)], shape
    assert B * C * S * 4 <= 36 * 2**20
  assert R.pick_nsplit(2, 2105348) > R.NT and R.pick_nsplit(2, 2105340) == 256  # a second trip, and a piece behind the last whole round
  assert R.pick_nsplit(1, 8396804) == 1024 and (8396804 // 4) // (8 * R.NT) == 1025  # the cap binds
  # the unrolled loop: (2, 3, 4100) once with a tail for thread 0; (1, 3, 16392) twice per block with a tail in threads 0 and 1 of block 0
  assert R.tail_start_piece(4100, 1) == 1024 and 4100 // 4 - 1024 == 1
  assert R.tail_start_piece(16392, 2) == 4096 and 16392 // 4 - 4096 == 2
  assert R.tail_start_piece(3072, 1) == 0


@pytest.mark.parametrize('shape,groups,step,span', R.GRID_CASES)
def test_grid_case_conditions(shape, groups, step, span):
  """grid_case asserts them itself (check_grid_case); here once more from outside, together with what the exact checks rest on: the
  exact statistics agree with the float64 definition, and the yardstick is evaluated on these inputs."""
  c = R.grid_case(shape, groups, 3, step, span)
  R.check_grid_case(c)
  mean, var, count = R.exact_statistics(c)
  fwd = R.forward(c['y'], c['gamma'], c['beta'], None, False, groups)
  assert count == fwd['count']
  assert np.abs(mean - fwd['mean'].numpy()).max() <= 1e-12 and np.abs(var - fwd['var'].numpy()).max() <= 1e-12
  for with_add in (False, True):
    pre = R.forward(c['y'], c['gamma'], c['beta'], c['add'] if with_add else None, False, groups)['pre']
    assert float(pre.abs().min()) >= 1e-3


@pytest.mark.parametrize('shape,groups', [(s, g) for s, g, _, _ in R.GRID_CASES if s[2] < 20000])
def test_random_case_conditions(shape, groups):
  c = R.random_case(shape, groups)
  for with_add in (False, True):
    pre = R.forward(c['y'], c['gamma'], c['beta'], c['add'] if with_add else None, False, groups)['pre']
    assert int((pre.abs() < 1e-5).sum()) == 0


@pytest.mark.parametrize('shape,groups,step,span', R.GRID_CASES)
def test_exact_checks_see_one_piece_lost_or_taken_twice(shape, groups, step, span):
  """A statistics loop that drops one 16-byte piece, or adds one twice -- at the first piece of a row, at the last, at the one that
  starts the tail loop -- moves sum (y - K)^2 by at least one unit of step^2.  The GPU tier compares the workspace totals as integers, so
  it sees one unit; and one unit is at least 16 float32 ulps of the partial sum of the block that took the piece (below 2^20 units)."""
  c = R.grid_case(shape, groups, 3, step, span)
  B, C, S = shape
  s0, s1 = R.exact_forward_sums(c)
  nsplit = R.pick_nsplit(C * groups, S)
  blk = R.block_of(S, nsplit)
  d = R._grouped_np(c['yi'], groups) - c['K'][:, None, :, None]
  places = sorted({0, S // 4 - 1, R.tail_start_piece(S, nsplit)})
  for g in range(groups):
    for ch in range(C):
      for piece in places:
        part = d[g, -1, ch, 4 * piece:4 * piece + 4]  # (the last sample of the group: the loops run once per sample)
        lost = int((part * part).sum())
        assert lost >= 1
        owner = int(blk[4 * piece])
        partial = float((d[g, :, ch][:, blk == owner]**2).sum())
        assert partial < 2**20
        for sign in (-1, +1):  # dropped, taken twice
          broken = partial + sign * lost
          assert abs(np.float32(broken) - np.float32(partial)) >= 16 * np.spacing(np.float32(partial))
          assert int(s1[g, ch]) + sign * lost != int(s1[g, ch])
