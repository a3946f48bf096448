"""Guard bands for the hand-off's backward (mode_multiview_handoff_bwd): no read or write outside the buffers it was given.

As tests/test_gpu_guard_bands_erp.py: the case is registered in the operator table of tests/test_gpu_guard_bands.py
(test_gpu_guard_bands.CASES, through its own case() helper) when this module is imported, so the ledger of
tests/test_guard_bands_host.py sees the entry whenever the suite is collected as a whole.  It runs here through
test_gpu_guard_bands.run_case (declared entries launched, guards intact under both fills, outputs bit-equal between the fills and
finite).

The case is the (2, 48, 24) shape of tests/test_gpu_handoff_grad.py (two frames: plane and key-plane offsets; 1152 pixels: a ragged
last block).  The disparities, the upstream gradient, the forward's keys and the three CSR arrays of the adjoint lists are all placed
between guards, so the key decode (a source index read from memory) and the list walk (ranges, targets and weights read from memory)
run between the 0x01 / 0x02 pattern fills.  gdisp is a torch.empty of the host code, which the guard allocator fills with a different
pattern in each of the two runs: bit equality between the fills also proves that every element is written."""
import pytest
import torch

import test_gpu_guard_bands as T

import handoff_ref as R
from utils import geometry as HG

HANDOFF_ENTRIES = ('mode_multiview_handoff', 'mode_multiview_handoff_bwd')
SHAPE = (2, 48, 24)


def _fresh_caches():
  """The adjoint lists are cached per device like the other tables: drop them, so that every run places them inside its guarded context."""
  T._fresh_caches()
  HG._adjoint_cache.clear()


def b_handoff_bwd(F_, H, W):
  disp, conf = R.inputs(F_, H, W, 7 + F_ + H)
  gout = torch.randn(F_, 12, H, W, generator=torch.Generator().manual_seed(11 + F_ + H))
  lists = HG._frames_adjoint(H, W, 'cpu')

  def run():
    _fresh_caches()
    d, c, g = T.P(disp), T.P(conf), T.P(gout)
    out, keys = HG.disp2depth_frames_gpu(d, c, return_keys=True)
    keys = T.P(keys.cpu())
    HG._adjoint_cache[(H, W, str(d.device))] = tuple(T.P(t) for t in lists)
    both = HG.disp2depth_frames_bwd(d, g, keys)
    alone = HG.disp2depth_frames_bwd(d, T.P(gout[:, 0::2].contiguous()), keys, depth_only=True)
    leaf = T.P(disp).requires_grad_(True)
    through, = torch.autograd.grad(HG.disp2depth_frames_gpu(leaf, c), leaf, g)
    return {'gdisp': both, 'depth_only': alone, 'autograd': through, 'keys': keys}

  def verify(out):
    assert torch.equal(out['gdisp'].view(torch.int32), out['depth_only'].view(torch.int32))
    assert torch.equal(out['gdisp'].view(torch.int32), out['autograd'].view(torch.int32))
    winner, v = R.decode_keys(out['keys'])
    ref = R.gradient(disp, winner, gout[:, 0::2], 'Deep360', torch.float64)
    # left out as in tests/test_gpu_handoff_grad.py: pixels at a clip boundary of the sine rule, winners at the 1000 cap
    skip = torch.stack([R.near_kink(disp[:, p], HG._baselines('Deep360')[p]) for p in range(6)], 1).view(F_, 6, H * W)
    for f, k in ((f, k) for f in range(F_) for k in range(3)):
      at_cap = (winner[f, k] >= 0) & ((v[f, k].double() - 1000).abs() <= 1)
      skip[f, 3 + k, winner[f, k][at_cap]] = True
    err = (out['gdisp'].double() - ref).abs()[~skip.view(F_, 6, H, W)]
    bound = 1e-4 * float(ref.abs().max())  # (the kernel's own bound is that of tests/test_gpu_handoff_grad.py; here: the right numbers at all)
    print('  gdisp: max err %.3e off the clip boundaries (bound %.3e), %d of %d elements not zero' %
          (float(err.max()), bound, int((out['gdisp'] != 0).sum()), out['gdisp'].numel()))
    assert float(err.max()) <= bound

  return run, verify


_FIRST = len(T.CASES)
T.case('multiview_handoff_bwd', list(HANDOFF_ENTRIES), b_handoff_bwd, SHAPE)
CASES = T.CASES[_FIRST:_FIRST + 1]


def test_the_case_declares_the_backward_entry():
  """CPU tier.  Together with the rest of the table it covers the launching ABI (the ledger of tests/test_guard_bands_host.py)."""
  assert set().union(*[c.entries for c in CASES]) == set(HANDOFF_ENTRIES)
  assert all(c in T.CASES for c in CASES) and len({c.id for c in T.CASES}) == len(T.CASES)
  import test_guard_bands_host as G
  assert set(HANDOFF_ENTRIES) <= G.launching_entries() and set(HANDOFF_ENTRIES) <= G._declared_entries()


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
def test_guarded_handoff_bwd(c, monkeypatch, stop_at_a_gpu_fault):
  rec, stats = T.run_case(c, monkeypatch)
  assert c.entries, 'every case declares the entries it is there to launch'
  missing = sorted(c.entries - set(rec.launched))
  assert not missing, 'declared but not launched: %s (launched: %s)' % (missing, sorted(rec.launched))
  assert set(rec.launched) <= set(HANDOFF_ENTRIES), sorted(rec.launched)
  assert rec.launched['mode_multiview_handoff_bwd'] >= 6  # three calls under each fill
  T.STATS['allocations'] += sum(stats['allocations'])
  T.STATS['launches'] += sum(rec.launched.values())
  T.STATS['cases'] += 1
  print('  %d guarded allocations, %d launching calls' % (sum(stats['allocations']), sum(rec.launched.values())))
  print('LAUNCHED %s %s' % (c.id, ' '.join(sorted(rec.launched))))
