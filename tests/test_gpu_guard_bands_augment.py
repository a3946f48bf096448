"""Guard bands for the colour augmentation entry (csrc/augment.hip: mode_images_u8_augment): no read or write outside the buffers it was
given.

As tests/test_gpu_guard_bands_optim.py: the case is registered in the operator table of tests/test_gpu_guard_bands.py
(test_gpu_guard_bands.CASES, through its own case() helper) when this module is imported -- this file sorts in front of
tests/test_guard_bands_host.py, so the ledger there sees the entry whenever the suite is collected as a whole.  It runs here through
test_gpu_guard_bands.run_case (declared entries launched, guards intact under both fills, outputs bit-equal between the fills and finite).

The case is the eight images of tests/augment_ref.py at 96 x 80 (1 920 quads: several blocks per image, a ragged last one; eight
partials per image) with every order, an image without operations and one with saturation alone.  The images, both parameter tables, the
slot table (two slots per image into eleven slots, some of them "none": one slot stays unwritten and must keep its sentinel) and the output are placed between
guards; the workspace and the means are torch.empty allocations of mode_hip/functional.py, which the guard allocator relocates and fills
with a different pattern in each of the two runs -- bit equality between the fills also proves that the fold reads only partials that
were written, and that images without a contrast step read none."""
import pytest
import torch

import augment_ref as A
import test_gpu_guard_bands as T

from mode_hip import functional as HF

AUGMENT_ENTRIES = ('mode_images_u8_augment',)
SLOTS = ((9, 3), (0, -1), (4, -1), (7, 12), (1, -1), (5, -1), (2, 6), (8, -1))  # image n -> its two slots (-1, 12: none); 10 stays unwritten
N_SLOTS = 11
SENTINEL = -7.0


def b_augment(H, W):
  images, rows, factors, shifts = A.case(H, W, A.FACTOR_SETS[2])
  ops, coef = A.tables(rows, factors, shifts)

  def run():
    out = T.PO(torch.full((N_SLOTS, 3, H, W), SENTINEL))
    res, means = HF.images_u8_augment(T.P(torch.from_numpy(images)), T.P(torch.from_numpy(ops)), T.P(torch.from_numpy(coef)),
                                      dst=T.P(torch.tensor(SLOTS, dtype=torch.int32)), out=out, return_means=True)
    assert res is out
    return {'out': out, 'means': means}

  def verify(out):
    means = out['means']
    want, infos = A.augment_batch(images, ops, coef, torch.float32, means=means)
    for n, row in enumerate(SLOTS):
      for s in row:
        if 0 <= s < N_SLOTS:
          assert torch.equal(out['out'][s], want[n]), (n, s)
      if infos[n]['mean'] is None:
        assert float(means[n]) == 0
      else:
        assert abs(float(means[n]) - infos[n]['grey_mean64']) <= 2.0 ** -24
    unwritten = set(range(N_SLOTS)) - {s for row in SLOTS for s in row}
    assert unwritten == {10}
    for s in unwritten:
      assert bool((out['out'][s] == SENTINEL).all())

  return run, verify


_FIRST = len(T.CASES)
T.case('images_u8_augment', list(AUGMENT_ENTRIES), b_augment, (96, 80))
CASES = T.CASES[_FIRST:_FIRST + 1]


def test_the_case_declares_the_augmentation_entry():
  """CPU tier.  Together with the rest of the table it covers the launching ABI (the ledger of tests/test_guard_bands_host.py)."""
  assert set().union(*[c.entries for c in CASES]) == set(AUGMENT_ENTRIES)
  assert all(c in T.CASES for c in CASES) and len({c.id for c in T.CASES}) == len(T.CASES)
  import test_guard_bands_host as G
  assert set(AUGMENT_ENTRIES) <= G.launching_entries() and set(AUGMENT_ENTRIES) <= G._declared_entries()
  import mode_hip
  new = {n for n in mode_hip.SIGNATURES if n.startswith('mode_images_u8_augment')}
  assert len(new) == 2 and new & G.launching_entries() == set(AUGMENT_ENTRIES)  # exactly the new launching entry; the other is the size query


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
def test_guarded_augment(c, monkeypatch, stop_at_a_gpu_fault):
  rec, stats = T.run_case(c, monkeypatch)
  assert c.entries, 'every case declares the entries it is there to launch'
  missing = sorted(c.entries - set(rec.launched))
  assert not missing, 'declared but not launched: %s (launched: %s)' % (missing, sorted(rec.launched))
  assert set(rec.launched) <= set(AUGMENT_ENTRIES), sorted(rec.launched)
  assert rec.launched['mode_images_u8_augment'] == 2  # once under each fill
  T.STATS['allocations'] += sum(stats['allocations'])
  T.STATS['launches'] += sum(rec.launched.values())
  T.STATS['cases'] += 1
  print('  %d guarded allocations, %d launching calls' % (sum(stats['allocations']), sum(rec.launched.values())))
  print('LAUNCHED %s %s' % (c.id, ' '.join(sorted(rec.launched))))
