"""Guard bands for the entries of include/mode_hip_mvphoto.h (csrc/mv_photometric.hip: mode_mvphoto_loss_fwd / _bwd): no read or write
outside the buffers they were given.

As tests/test_gpu_guard_bands_selfsup.py, this file does NOT register its case in test_gpu_guard_bands.CASES: the ledger of
tests/test_guard_bands_host.py requires every registered entry to be in mode_hip.LAUNCHING, the launching set of the first header, and
these entries are declared in the third.  It calls guard_bands.under_two_fills itself, with a recording stand-in for the library handle
that counts the names in mode_hip.MVPHOTO_LAUNCHING.

The case is 1 x 70 x 37 with S = 2 (the third case of tests/mvphoto_ref.py): five ragged tile rows and two ragged tile columns, an odd
width, gathers that wrap along H in both sources.  The reference image, the sources and the depth map are placed between guards; the
winners, the statistics, the loss, the slab workspace and the gradient are allocations of mode_hip/functional.py, which the guard
allocator relocates and fills with a different pattern in each of the two runs -- bit equality between the fills also proves that the
fold reads only slab columns that were written and that every winner byte and every gradient element is written."""
import collections

import pytest
import torch

import guard_bands as GB
import mvphoto_ref as M

import mode_hip
from mode_hip import functional as HF

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASE = M.CASES[2]


class RecordingLib(object):
  """Stands in for the ctypes handle: counts the calls of every launching entry of the third header."""

  def __init__(self, real):
    self._real, self.launched = real, collections.Counter()

  def __getattr__(self, name):
    fn = getattr(self._real, name)
    if name not in mode_hip.MVPHOTO_LAUNCHING:
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
  ref, src, depth, poses = M.make_case(*CASE)
  r, s = GB.place(ref.to(DEV)), GB.place(src.to(DEV))
  d = GB.place(depth.to(DEV)).detach().requires_grad_(True)
  loss, stats, win = HF.mv_photometric_loss(r, s, d, poses, return_stats=True, return_win=True)
  loss.backward()
  return {'loss': loss.detach(), 'stats': stats, 'win': win, 'g': d.grad}


def test_guarded_mvphoto(monkeypatch):
  assert CASE == (1, 70, 37, 2)
  real = mode_hip.lib()
  rec = RecordingLib(real)
  monkeypatch.setattr(mode_hip, '_lib', rec)
  try:
    leaves, stats = GB.under_two_fills(_run)
  finally:
    monkeypatch.setattr(mode_hip, '_lib', real)
  assert set(rec.launched) == set(mode_hip.MVPHOTO_LAUNCHING) and len(mode_hip.MVPHOTO_LAUNCHING) == 2, sorted(rec.launched)
  assert rec.launched['mode_mvphoto_loss_fwd'] == rec.launched['mode_mvphoto_loss_bwd'] == 2  # once under each fill
  print('  %d guarded allocations, %d launching calls' % (sum(stats['allocations']), sum(rec.launched.values())))
  out = dict(leaves)
  # within the parity bound of tests/test_gpu_mvphoto.py: winners and counts exactly, loss and gradient within 4 x the yardstick
  l64, i64, g64 = M.reference(CASE, torch.float64)
  l32, _, g32 = M.reference(CASE, torch.float32)
  assert torch.equal(out["out['win']"].cpu(), i64['win']) and float(out["out['stats']"][0]) == i64['N']

  def within(got, a32, b64):
    yard, scale = M.yardstick(a32, b64)
    assert M.error(got.cpu(), b64, scale) <= 4 * yard

  within(out["out['loss']"], l32, l64)
  within(out["out['g']"], g32, g64)
