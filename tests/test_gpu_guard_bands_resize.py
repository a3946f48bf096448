"""Guard bands for the any-size pair ingest (csrc/resize.hip: mode_images_u8_resize_pil, mode_disp_resize_nearest): no read or write
outside the buffers they were given.

As tests/test_gpu_guard_bands_augment.py: the cases are registered in the operator table of tests/test_gpu_guard_bands.py
(test_gpu_guard_bands.CASES, through its own case() helper) when this module is imported -- this file sorts in front of
tests/test_guard_bands_host.py, so the ledger there sees the entries whenever the suite is collected as a whole.  They run here through
test_gpu_guard_bands.run_case (declared entries launched, guards intact under both fills, outputs bit-equal between the fills and finite).

Both cases are 37 x 23 -> 50 x 9 -- rows of 69 bytes, images of 2 553: nothing is a multiple of 4, one axis grows and the other
shrinks -- with a window per image, one of them in the bottom right corner, where the last taps of both tables end at the last source
row and column.  The images, both tables, the lookup table and the windows are placed between guards; both outputs and the workspace
(the 8-bit result of the horizontal pass) are torch.empty allocations of mode_hip/functional.py, which the guard allocator relocates
and fills with a different pattern in each of the two runs -- bit equality between the fills also proves that the vertical pass reads
only rows of the workspace that the horizontal pass wrote for the window."""
import numpy as np
import pytest
import torch

import resize_ref as R
import test_gpu_guard_bands as T

from dataloader import deep360_loader as L
from dataloader import gpu_ingest as G
from dataloader import preprocess
from mode_hip import functional as HF

RESIZE_ENTRIES = ('mode_images_u8_resize_pil', 'mode_disp_resize_nearest')
CROP = (20, 5)
WINDOWS = ((0, 0), (30, 4), (13, 2))  # of 20 x 5 in the 50 x 9 image: top-left corner, bottom-right corner, interior


def b_images(Hs, Ws, H, W):
  images = np.stack([R.image('binary' if n == 1 else 'random', Hs, Ws, seed=n) for n in range(len(WINDOWS))])

  def run():
    u8, f32 = HF.images_u8_resize_pil(T.P(torch.from_numpy(images)), (H, W), T.P(G.resize_table_rows(Ws, W)), T.P(G.resize_table_rows(Hs, H)),
                                      lut=T.P(preprocess.norm_table()), windows=T.P(torch.tensor(WINDOWS, dtype=torch.int32)), crop=CROP,
                                      want_f32=True)
    return {'u8': u8, 'f32': f32}

  def verify(out):
    transform = preprocess.get_transform_stage1(augment=False)
    assert tuple(out['u8'].shape) == (len(WINDOWS),) + CROP + (3,) and tuple(out['f32'].shape) == (len(WINDOWS), 3) + CROP
    for n, (top, left) in enumerate(WINDOWS):
      want = R.pil_resize(images[n], H, W)[top:top + CROP[0], left:left + CROP[1]]
      assert np.array_equal(out['u8'][n].numpy(), want), n
      assert torch.equal(out['f32'][n], transform(want)), n

  return run, verify


def b_disp(Hs, Ws, H, W):
  r = np.random.RandomState(5)
  disp = (r.rand(len(WINDOWS), Hs, Ws) * 40).astype(np.float32)
  disp[r.rand(*disp.shape) < 0.2] = 0.0

  def run():
    rows, cols = preprocess.nearest_index_table(Hs, H), preprocess.nearest_index_table(Ws, W)
    out = HF.disp_resize_nearest(T.P(torch.from_numpy(disp)), (H, W), T.P(torch.from_numpy(rows)), T.P(torch.from_numpy(cols)), W / Ws,
                                 windows=T.P(torch.tensor(WINDOWS, dtype=torch.int32)), crop=CROP)
    return {'disp': out}

  def verify(out):
    for n, (top, left) in enumerate(WINDOWS):
      want = (L.resize_nearest(disp[n], W, H) * (W / Ws))[top:top + CROP[0], left:left + CROP[1]]
      assert want.dtype == np.float32 and np.array_equal(out['disp'][n].numpy().view(np.int32), want.view(np.int32)), n

  return run, verify


_FIRST = len(T.CASES)
T.case('images_u8_resize_pil', [RESIZE_ENTRIES[0]], b_images, (37, 23, 50, 9))
T.case('disp_resize_nearest', [RESIZE_ENTRIES[1]], b_disp, (37, 23, 50, 9))
CASES = T.CASES[_FIRST:_FIRST + 2]


def test_the_cases_declare_exactly_the_new_entries():
  """CPU tier.  Together with the rest of the table they cover the launching ABI (the ledger of tests/test_guard_bands_host.py)."""
  assert set().union(*[c.entries for c in CASES]) == set(RESIZE_ENTRIES)
  assert all(c in T.CASES for c in CASES) and len({c.id for c in T.CASES}) == len(T.CASES)
  import test_guard_bands_host as H
  assert set(RESIZE_ENTRIES) <= H.launching_entries() and set(RESIZE_ENTRIES) <= H._declared_entries()
  import mode_hip
  new = {n for n in mode_hip.SIGNATURES if n.startswith('mode_images_u8_resize_pil') or n.startswith('mode_disp_resize')}
  assert len(new) == 3 and new & H.launching_entries() == set(RESIZE_ENTRIES)  # exactly the two launching entries; the third is the size query


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
def test_guarded_resize(c, monkeypatch, stop_at_a_gpu_fault):
  rec, stats = T.run_case(c, monkeypatch)
  assert c.entries, 'every case declares the entries it is there to launch'
  missing = sorted(c.entries - set(rec.launched))
  assert not missing, 'declared but not launched: %s (launched: %s)' % (missing, sorted(rec.launched))
  assert set(rec.launched) == set(c.entries), sorted(rec.launched)
  assert sum(rec.launched.values()) == 2  # once under each fill
  T.STATS['allocations'] += sum(stats['allocations'])
  T.STATS['launches'] += sum(rec.launched.values())
  T.STATS['cases'] += 1
  print('  %d guarded allocations, %d launching calls' % (sum(stats['allocations']), sum(rec.launched.values())))
  print('LAUNCHED %s %s' % (c.id, ' '.join(sorted(rec.launched))))
