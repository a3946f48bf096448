"""Guard bands for the entry of include/mode_hip_mvpose.h (csrc/mv_pose_grad.hip: mode_mvpose_grad): no read or write outside the
buffers it was given.

As tests/test_gpu_guard_bands_mvphoto.py, this file does NOT register its case in test_gpu_guard_bands.CASES: the ledger of
tests/test_guard_bands_host.py requires every registered entry to be in mode_hip.LAUNCHING, the launching set of the first header, and
this entry is declared in the fourth.  It calls guard_bands.under_two_fills itself, with a recording stand-in for the library handle
that counts the names in mode_hip.MVPOSE_LAUNCHING.

The case is 1 x 70 x 37 with S = 2 and perturbed poses (the third case of tests/mvpose_ref.py): five ragged tile rows and two ragged
tile columns, an odd width, gathers that wrap along H in both sources.  The reference image, the sources and the depth map are placed
between guards; the winners, the statistics, the slab workspaces and the S x 12 gradient are allocations of mode_hip/functional.py,
which the guard allocator relocates and fills with a different pattern in each of the two runs -- bit equality between the fills also
proves that the fold reads only slab columns that were written (a source without a window in a tile writes zeros there) and that
every element of gposes is written."""
import collections

import pytest
import torch

import guard_bands as GB
import mvpose_ref as P

import mode_hip
from mode_hip import functional as HF

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASE = P.CASES[2]


class RecordingLib(object):
  """Stands in for the ctypes handle: counts the calls of the launching entry of the fourth header."""

  def __init__(self, real):
    self._real, self.launched = real, collections.Counter()

  def __getattr__(self, name):
    fn = getattr(self._real, name)
    if name not in mode_hip.MVPOSE_LAUNCHING:
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
  ref, src, depth, poses = P.make_case(*CASE)
  r, s, d = GB.place(ref.to(DEV)), GB.place(src.to(DEV)), GB.place(depth.to(DEV))
  pt = torch.from_numpy(poses).clone().requires_grad_(True)
  loss, stats, win = HF.mv_photometric_loss(r, s, d, pt, return_stats=True, return_win=True)
  loss.backward()
  return {'stats': stats, 'win': win, 'g': pt.grad}


def test_guarded_mvpose(monkeypatch):
  assert CASE == (1, 70, 37, 2)
  real = mode_hip.lib()
  rec = RecordingLib(real)
  monkeypatch.setattr(mode_hip, '_lib', rec)
  try:
    leaves, stats = GB.under_two_fills(_run)
  finally:
    monkeypatch.setattr(mode_hip, '_lib', real)
  assert dict(rec.launched) == {'mode_mvpose_grad': 2} and mode_hip.MVPOSE_LAUNCHING == {'mode_mvpose_grad'}  # once under each fill
  print('  %d guarded allocations, %d launching calls' % (sum(stats['allocations']), sum(rec.launched.values())))
  out = dict(leaves)
  # within the parity bound of tests/test_gpu_mvpose.py: winners and counts exactly, the gradient within 4 x the yardstick
  _, i64, g64 = P.reference(CASE, torch.float64)
  _, _, g32 = P.reference(CASE, torch.float32)
  assert torch.equal(out["out['win']"].cpu(), i64['win']) and float(out["out['stats']"][0]) == i64['N']
  yard, scale = P.yardstick(g32, g64)
  assert P.error(out["out['g']"].cpu(), g64, scale) <= 4 * yard
