"""Guard bands for the self-supervised stereo loss (csrc/photometric.hip: mode_photometric_loss_fwd, mode_photometric_loss_bwd): no
read or write outside the buffers they were given.

As tests/test_gpu_guard_bands_augment.py: the case is registered in the operator table of tests/test_gpu_guard_bands.py
(test_gpu_guard_bands.CASES, through its own case() helper) when this module is imported -- this file sorts in front of
tests/test_guard_bands_host.py, so the ledger there sees the entries whenever the suite is collected as a whole.  It runs here through
test_gpu_guard_bands.run_case (declared entries launched, guards intact under both fills, outputs bit-equal between the fills and finite).

The case is 70 x 37 with K = 2 (tests/photometric_ref.py's third case): five tile rows and two tile columns, both ragged, rows that
wrap at both ends of H and disparities that point outside [0, W - 1] on either side.  Both images and the two disparity maps are
placed between guards; the stacked maps, the statistics, the loss, the slab workspace and gdisp are allocations of mode_hip/functional.py,
which the guard allocator relocates and fills with a different pattern in each of the two runs -- bit equality between the fills also
proves that the fold reads only slab columns that were written and that gdisp is written everywhere."""
import pytest
import torch

import photometric_ref as R
import test_gpu_guard_bands as T

from mode_hip import functional as HF

PHOTOMETRIC_ENTRIES = ('mode_photometric_loss_fwd', 'mode_photometric_loss_bwd')


def b_photometric(B, H, W, K, maxd):
  case = (B, H, W, K, maxd)
  left, right, disps = R.make_case(*case)

  def run():
    ds = [T.P(d).detach().requires_grad_(True) for d in disps]
    loss, stats = HF.photometric_loss(T.P(left), T.P(right), ds, R.WEIGHTS[:K], return_stats=True)
    loss.backward()
    return {'loss': loss.detach(), 'stats': stats, 'g': [d.grad for d in ds]}

  def verify(out):
    """The bounds of tests/test_gpu_photometric.py: counts exactly, loss and gradient within 4 x the float32 restatement's own error."""
    l64, s64, g64 = R.reference(case, torch.float64)
    l32, _, g32 = R.reference(case, torch.float32)
    assert torch.equal(out['stats'][:, 0], s64[:, 0])
    assert abs(float(out['loss'].double()) - float(l64)) <= 4 * abs(float(l32) - float(l64))
    for k in range(K):
      got = out['g[%d]' % k].double()
      assert float((got - g64[k]).abs().max()) <= 4 * float((g32[k].double() - g64[k]).abs().max()), k

  return run, verify


_FIRST = len(T.CASES)
T.case('photometric_loss', list(PHOTOMETRIC_ENTRIES), b_photometric, R.CASES[2])
CASES = T.CASES[_FIRST:_FIRST + 1]


def test_the_case_declares_the_photometric_entries():
  """CPU tier.  Together with the rest of the table it covers the launching ABI (the ledger of tests/test_guard_bands_host.py)."""
  assert R.CASES[2][1:4] == (70, 37, 2)
  assert set().union(*[c.entries for c in CASES]) == set(PHOTOMETRIC_ENTRIES)
  assert all(c in T.CASES for c in CASES) and len({c.id for c in T.CASES}) == len(T.CASES)
  import test_guard_bands_host as G
  assert set(PHOTOMETRIC_ENTRIES) <= G.launching_entries() and set(PHOTOMETRIC_ENTRIES) <= G._declared_entries()
  import mode_hip
  new = {n for n in mode_hip.SIGNATURES if n.startswith('mode_photometric_')}
  assert len(new) == 3 and new & G.launching_entries() == set(PHOTOMETRIC_ENTRIES)  # the two launching entries; the third is the size query


@pytest.fixture
def stop_at_a_gpu_fault():
  """As test_gpu_guard_bands._stop_at_a_gpu_fault (not autouse here: this file has a CPU-tier test): if the device no longer answers
  after a test, the session ends there."""
  yield
  try:
    torch.cuda.synchronize()
  except RuntimeError as e:
    pytest.exit('the GPU reported an error after this test; nothing more is started on it: %s' % e, returncode=3)


@pytest.mark.gpu
@pytest.mark.parametrize('c', CASES, ids=[c.id for c in CASES])
def test_guarded_photometric(c, monkeypatch, stop_at_a_gpu_fault):
  rec, stats = T.run_case(c, monkeypatch)
  assert c.entries, 'every case declares the entries it is there to launch'
  missing = sorted(c.entries - set(rec.launched))
  assert not missing, 'declared but not launched: %s (launched: %s)' % (missing, sorted(rec.launched))
  assert set(rec.launched) == set(PHOTOMETRIC_ENTRIES), sorted(rec.launched)
  assert all(n == 2 for n in rec.launched.values())  # once under each fill
  T.STATS['allocations'] += sum(stats['allocations'])
  T.STATS['launches'] += sum(rec.launched.values())
  T.STATS['cases'] += 1
  print('  %d guarded allocations, %d launching calls' % (sum(stats['allocations']), sum(rec.launched.values())))
  print('LAUNCHED %s %s' % (c.id, ' '.join(sorted(rec.launched))))
