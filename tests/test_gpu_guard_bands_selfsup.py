"""Guard bands for the entries of include/mode_hip_selfsup.h (csrc/lr_consistency.hip: mode_lr_consistency_fwd / _bwd;
csrc/photometric.hip: mode_selfsup_view_loss_fwd / _bwd): no read or write outside the buffers they were given.

Unlike the other guard-band files this one does NOT register its case in test_gpu_guard_bands.CASES: the ledger of
tests/test_guard_bands_host.py requires every registered entry to be in mode_hip.LAUNCHING, the launching set of the first header, and
these entries are declared in the second.  It calls guard_bands.under_two_fills itself, with a recording stand-in for the library
handle that counts the names in mode_hip.SELFSUP_LAUNCHING.

The case is 70 x 37 with K = 2 (the third case of tests/selfsup_ref.py): a row length that is no multiple of anything, five ragged tile
rows and two ragged tile columns for the view loss, disparities that point outside [0, W - 1] on either side and a few negative ones.
Both images and the four maps are placed between guards; the stacked maps, the masks, the statistics, the losses, the slab workspaces
and the gradients are allocations of mode_hip/functional.py, which the guard allocator relocates and fills with a different pattern in
each of the two runs -- bit equality between the fills also proves that the folds read only slab columns that were written, that every
mask byte and every gradient element is written, and that the view loss reads no mask byte outside its plane."""
import collections

import pytest
import torch

import guard_bands as GB
import selfsup_ref as S

import mode_hip
from mode_hip import functional as HF

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASE = S.CASES[2]


class RecordingLib(object):
  """Stands in for the ctypes handle: counts the calls of every launching entry of the second header."""

  def __init__(self, real):
    self._real, self.launched = real, collections.Counter()

  def __getattr__(self, name):
    fn = getattr(self._real, name)
    if name not in mode_hip.SELFSUP_LAUNCHING:
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
  left, right, dls, drs = S.make_case(*CASE)
  K = len(dls)
  tau, dmax = S.params(CASE)
  wts = S.WEIGHTS[:K]
  l, r = GB.place(left.to(DEV)), GB.place(right.to(DEV))
  ls = [GB.place(d.to(DEV)).detach().requires_grad_(True) for d in dls]
  rs = [GB.place(d.to(DEV)).detach().requires_grad_(True) for d in drs]
  lr, masks, lr_stats = HF.lr_consistency(ls, rs, wts, tau=tau, dmax=dmax, return_masks=True, return_stats=True)
  lr.backward()
  out = {'lr': lr.detach(), 'masks': masks, 'lr_stats': lr_stats, 'gdl': [d.grad for d in ls], 'gdr': [d.grad for d in rs]}
  for name, own, other, maps, view, m in (('left', l, r, dls, 'left', masks[0]), ('right', r, l, drs, 'right', masks[1])):
    ds = [GB.place(d.to(DEV)).detach().requires_grad_(True) for d in maps]
    loss, stats = HF.photometric_loss(own, other, ds, wts, return_stats=True, view=view, masks=m)
    loss.backward()
    out[name] = {'loss': loss.detach(), 'stats': stats, 'g': [d.grad for d in ds]}
  return out


def test_guarded_selfsup(monkeypatch):
  assert CASE[1:4] == (70, 37, 2)
  real = mode_hip.lib()
  rec = RecordingLib(real)
  monkeypatch.setattr(mode_hip, '_lib', rec)
  try:
    leaves, stats = GB.under_two_fills(_run)
  finally:
    monkeypatch.setattr(mode_hip, '_lib', real)
  assert set(rec.launched) == set(mode_hip.SELFSUP_LAUNCHING) and len(mode_hip.SELFSUP_LAUNCHING) == 4, sorted(rec.launched)
  assert rec.launched['mode_lr_consistency_fwd'] == rec.launched['mode_lr_consistency_bwd'] == 2  # once under each fill
  assert rec.launched['mode_selfsup_view_loss_fwd'] == rec.launched['mode_selfsup_view_loss_bwd'] == 4  # both views under each fill
  print('  %d guarded allocations, %d launching calls' % (sum(stats['allocations']), sum(rec.launched.values())))
  out = dict(leaves)
  K = CASE[3]
  # within the parity bound of tests/test_gpu_selfsup.py: masks and counts exactly, losses and gradients within 4 x the yardstick
  l64, s64, m64, gl64, gr64 = S.lr_reference(CASE, torch.float64)
  l32, _, _, gl32, gr32 = S.lr_reference(CASE, torch.float32)
  assert torch.equal(out["out['masks']"].bool(), m64)
  assert torch.equal(out["out['lr_stats']"][..., 0], s64[..., 0]) and torch.equal(out["out['lr_stats']"][..., 2], s64[..., 2])

  def within(got, a32, b64):
    yard, scale = S.yardstick(a32, b64)
    assert S.error(got, b64, scale) <= 4 * yard

  within(out["out['lr']"], l32, l64)
  for k in range(K):
    within(out["out['gdl'][%d]" % k], gl32[k], gl64[k])
    within(out["out['gdr'][%d]" % k], gr32[k], gr64[k])
  for view, name in enumerate(('left', 'right')):
    v64, v32 = S.view_reference(CASE, torch.float64, view, True), S.view_reference(CASE, torch.float32, view, True)
    assert torch.equal(out["out['%s']['stats']" % name][:, 0], v64[1][:, 0])
    within(out["out['%s']['loss']" % name], v32[0], v64[0])
    for k in range(K):
      within(out["out['%s']['g'][%d]" % (name, k)], v32[2][k], v64[2][k])
