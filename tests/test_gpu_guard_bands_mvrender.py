"""Guard bands for the launching entry of include/mode_hip_mvrender.h (csrc/mv_render.hip: mode_mv_render): no read or write outside
the buffers it was given.

As tests/test_gpu_guard_bands_mvvis.py, this file does NOT register its case in test_gpu_guard_bands.CASES: the ledger of
tests/test_guard_bands_host.py requires every registered entry to be in mode_hip.LAUNCHING, the launching set of the first header, and
this entry is declared in the sixth.  It calls guard_bands.under_two_fills itself, with a recording stand-in for the library handle
that counts the names in mode_hip.MVRENDER_LAUNCHING.

The case is 1 x 70 x 37 with T = 2 (the third case of tests/mvrender_ref.py), C = 3, fill = 1, both colour modes: an odd width, landing
pixels that wrap along H, the resolve reading the eight neighbours of target pixels in the first and last rows and columns, and the
bilinear's second row and column at the wrap and at W - 2.  The image and the depth map are placed between guards; out, hit, range,
index and the four-part workspace are allocations of mode_hip/functional.py, which the guard allocator relocates and fills with a
different pattern in each of the two runs -- bit equality between the fills also proves that the owners' launch and the resolve read
only keys, ranges, landing indices and owners that the launches before them wrote."""
import collections

import pytest
import torch

import guard_bands as GB
import mvphoto_ref as M
import mvrender_ref as R

import mode_hip
from mode_hip import functional as HF

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASE = R.CASES[2]


class RecordingLib(object):
  """Stands in for the ctypes handle: counts the calls of the launching entries of the sixth header."""

  def __init__(self, real):
    self._real, self.launched = real, collections.Counter()

  def __getattr__(self, name):
    fn = getattr(self._real, name)
    if name not in mode_hip.MVRENDER_LAUNCHING:
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
  image, depth, poses = R.make_case(CASE)
  img, d = GB.place(image.to(DEV)), GB.place(depth.to(DEV))
  out = {}
  for mode in ('splat', 'resample'):
    o, rng, hit, index = HF.mv_render(img, d, poses, fill=1, mode=mode, return_range=True, return_hit=True, return_index=True)
    # (range holds +inf where nothing is seen, on purpose: its finite part and its pattern are returned apart)
    out[mode] = {'out': o, 'hit': hit, 'index': index, 'empty': torch.isinf(rng), 'range': torch.where(torch.isinf(rng), torch.zeros_like(rng), rng)}
  return out


def test_guarded_mvrender(monkeypatch):
  assert CASE == (1, 70, 37, 2)
  real = mode_hip.lib()
  rec = RecordingLib(real)
  monkeypatch.setattr(mode_hip, '_lib', rec)
  try:
    leaves, stats = GB.under_two_fills(_run)
  finally:
    monkeypatch.setattr(mode_hip, '_lib', real)
  # under each fill: one call per colour mode
  assert dict(rec.launched) == {'mode_mv_render': 4}
  assert set(rec.launched) == mode_hip.MVRENDER_LAUNCHING
  print('  %d guarded allocations, %d launching calls' % (sum(stats['allocations']), sum(rec.launched.values())))
  got = dict(leaves)
  # and the results are the restatement's
  want64, want32 = R.reference(CASE, 0.05, 1), R.reference(CASE, 0.05, 1, dtype=torch.float32)
  for mode in ('splat', 'resample'):
    g = {k: got["out['%s']['%s']" % (mode, k)] for k in ('out', 'hit', 'index', 'empty', 'range')}
    assert torch.equal(g['hit'], want64['hit'] if mode == 'resample' else want64['hit'] & (R.DIRECT | R.FILLED))
    assert torch.equal(g['index'], want64['index']) and torch.equal(g['empty'], torch.isinf(want64['range']))
    assert 0 < int(g['empty'].sum()) < g['empty'].numel()
  image = R.make_case(CASE)[0]
  src = want64['index'].long().clamp(min=0).reshape(1, 1, -1).expand(1, 3, -1)
  copied = image.reshape(1, 3, -1).gather(2, src).reshape(1, 3, 2, 70, 37).permute(0, 2, 1, 3, 4)
  copied = torch.where((want64['index'] >= 0).unsqueeze(2), copied, torch.zeros(()))
  assert torch.equal(got["out['splat']['out']"], copied)
  yard, scale = M.yardstick(want32['out'], want64['out'])
  assert M.error(got["out['resample']['out']"], want64['out'], scale) <= 4 * yard
