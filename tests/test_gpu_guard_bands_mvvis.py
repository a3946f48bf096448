"""Guard bands for the two launching entries of include/mode_hip_mvvis.h (csrc/mv_visibility.hip: mode_mv_visibility; the masked
instantiation of csrc/mv_photometric.hip: mode_mvphoto_loss_fwd_masked): no read or write outside the buffers they were given.

As tests/test_gpu_guard_bands_mvpose.py, this file does NOT register its case in test_gpu_guard_bands.CASES: the ledger of
tests/test_guard_bands_host.py requires every registered entry to be in mode_hip.LAUNCHING, the launching set of the first header, and
these entries are declared in the fifth.  It calls guard_bands.under_two_fills itself, with a recording stand-in for the library handle
that counts the names in mode_hip.MVVIS_LAUNCHING.

The case is 1 x 70 x 37 with S = 2 (the third case of tests/mvvis_ref.py): five ragged tile rows and two ragged tile columns, an odd
width, landing pixels that wrap along H in both sources, at radius 1 so that the resolve reads the eight neighbours of landing pixels
in the first and last rows and columns.  The depth map, the images and (for the loss) the masks are placed between guards; vis, zbuf,
the three-part workspace of the visibility, the winners, the statistics and the slab are allocations of mode_hip/functional.py, which
the guard allocator relocates and fills with a different pattern in each of the two runs -- bit equality between the fills also
proves that the resolve reads only keys, ranges and landing indices that the two launches before it wrote."""
import collections

import pytest
import torch

import guard_bands as GB
import mvvis_ref as V

import mode_hip
from mode_hip import functional as HF

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASE = V.CASES[2]


class RecordingLib(object):
  """Stands in for the ctypes handle: counts the calls of the launching entries of the fifth header."""

  def __init__(self, real):
    self._real, self.launched = real, collections.Counter()

  def __getattr__(self, name):
    fn = getattr(self._real, name)
    if name not in mode_hip.MVVIS_LAUNCHING:
      return fn

    def call(*args):
      self.launched[name] += 1
      return fn(*args)

    return call


@pytest.fixture(autouse=True)
def _stop_at_a_gpu_fault():
  """As tests/test_gpu_guard_bands.py: if the device no longer answers after a test, the session ends there."""
  yield
  try:
    torch.cuda.synchronize()
  except RuntimeError as e:
    pytest.exit('the GPU reported an error after this test; nothing more is started on it: %s' % e, returncode=3)


def _run():
  ref, src, depth, poses = V.make_case(*CASE)
  r, s, d = GB.place(ref.to(DEV)), GB.place(src.to(DEV)), GB.place(depth.to(DEV))
  near, zbuf = HF.mv_visibility(d, poses, radius=1, return_zbuf=True)
  vis = HF.mv_visibility(d, poses)
  d = d.detach().requires_grad_(True)
  loss, stats, win = HF.mv_photometric_loss(r, s, d, poses, return_stats=True, return_win=True, masks=GB.place(vis))
  loss.backward()
  # (zbuf holds +inf where nothing lands, on purpose: its finite part and its pattern are returned apart)
  return {'near': near, 'vis': vis, 'empty': torch.isinf(zbuf), 'zbuf': torch.where(torch.isinf(zbuf), torch.zeros_like(zbuf), zbuf),
          'loss': loss.detach(), 'stats': stats, 'win': win, 'g': d.grad}


def test_guarded_mvvis(monkeypatch):
  assert CASE == (1, 70, 37, 2)
  real = mode_hip.lib()
  rec = RecordingLib(real)
  monkeypatch.setattr(mode_hip, '_lib', rec)
  try:
    leaves, stats = GB.under_two_fills(_run)
  finally:
    monkeypatch.setattr(mode_hip, '_lib', real)
  # under each fill: the visibility twice, the masked forward once
  assert dict(rec.launched) == {'mode_mv_visibility': 4, 'mode_mvphoto_loss_fwd_masked': 2}
  assert set(rec.launched) == mode_hip.MVVIS_LAUNCHING
  print('  %d guarded allocations, %d launching calls' % (sum(stats['allocations']), sum(rec.launched.values())))
  out = dict(leaves)
  # and the results are the restatement's: the masks and the winners exactly
  assert torch.equal(out["out['vis']"], V.reference_visibility(CASE)['vis'])
  assert torch.equal(out["out['near']"], V.reference_visibility(CASE, 0.05, 1)['vis'])
  assert torch.equal(out["out['empty']"], torch.isinf(V.reference_visibility(CASE)['zbuf']))
  _, i64, g64 = V.reference(CASE, torch.float64)
  _, _, g32 = V.reference(CASE, torch.float32)
  assert torch.equal(out["out['win']"], i64['win']) and float(out["out['stats']"][0]) == i64['N']
  yard, scale = V.M.yardstick(g32, g64)
  assert V.M.error(out["out['g']"], g64, scale) <= 4 * yard
