"""Guard bands for the three entries of the confidence gradient (mode_head_bwd_conf, mode_multiview_handoff_bwd_full,
mode_decimate2_bwd): no read or write outside the buffers they were given.

As tests/test_gpu_guard_bands_handoff.py: the case is registered in the operator table of tests/test_gpu_guard_bands.py
(test_gpu_guard_bands.CASES, through its own case() helper) when this module is imported, so the ledger of
tests/test_guard_bands_host.py sees the entries whenever the suite is collected as a whole.  It runs here through
test_gpu_guard_bands.run_case (declared entries launched, guards intact under both fills, outputs bit-equal between the fills and
finite).

One case for the three: the hand-off at the (2, 48, 24) shape of tests/test_gpu_handoff_grad.py (two frames: plane and key-plane
offsets; 1152 pixels: a ragged last block) with the disparities, the upstream gradient, the forward's keys and the CSR arrays of the
adjoint lists between guards; the head at (1, 12, 5, 7) x 4 (odd sizes: a ragged last row block) with the logits, the forward's outputs
and both upstream gradients between guards; the decimation at an odd size, where the last quad of the flat output is a partial one.
gdisp, gconf, glogits and gin are torch.empty of the host code, which the guard allocator fills with a different pattern in each of
the two runs: bit equality between the fills also proves that every element is written."""
import pytest
import torch

import test_gpu_guard_bands as T

import conf_grad_ref as C
import handoff_ref as R
from mode_hip import functional as HF
from utils import geometry as HG

NEW_ENTRIES = ('mode_head_bwd_conf', 'mode_multiview_handoff_bwd_full', 'mode_decimate2_bwd')
FORWARDS = ('mode_head_fwd', 'mode_multiview_handoff')  # what makes the forward's outputs the backward entries read
HANDOFF, HEAD, DECIMATE = (2, 48, 24), (1, 12, 5, 7, 4), (3, 5, 7)


def _fresh_caches():
  T._fresh_caches()
  HG._adjoint_cache.clear()


def b_conf_grad():
  F_, H, W = HANDOFF
  disp, conf = R.inputs(F_, H, W, 7 + F_ + H)
  gout = torch.randn(F_, 12, H, W, generator=torch.Generator().manual_seed(11 + F_ + H))
  lists = HG._frames_adjoint(H, W, 'cpu')
  B, D4, H4, W4, ratio = HEAD
  size = (D4 * ratio, H4 * ratio, W4 * ratio)
  lg, gp = T._rand((B, 1, D4, H4, W4), 61, 3.0), T._rand((B, 1) + size[1:], 62)
  gc, zeroed = C.masked_gconf(lg, T._rand((B, 1) + size[1:], 63), size)
  gy = T._rand(DECIMATE[:-2] + ((DECIMATE[-2] + 1) // 2, (DECIMATE[-1] + 1) // 2), 64)

  def run():
    _fresh_caches()
    d, c, g = T.P(disp), T.P(conf), T.P(gout)
    out, keys = HG.disp2depth_frames_gpu(d, c, return_keys=True)
    keys = T.P(keys.cpu())
    HG._adjoint_cache[(H, W, str(d.device))] = tuple(T.P(t) for t in lists)
    gdisp, gconf = HG.disp2depth_frames_bwd(d, g, keys, conf_grad=True)
    ld, lc = T.P(disp).requires_grad_(True), T.P(conf).requires_grad_(True)
    through = torch.autograd.grad(HG.disp2depth_frames_gpu(ld, lc, conf_grad=True), (ld, lc), g)
    logits = T.P(lg)
    pred, cf = HF.head_fwd(logits, size, with_confidence=True)
    gl = HF.head_bwd_conf(logits, T.P(pred.cpu()), T.P(cf.cpu()), T.P(gp), T.P(gc), size)
    return {'gdisp': gdisp, 'gconf': gconf, 'autograd_d': through[0], 'autograd_c': through[1], 'keys': keys, 'gl': gl,
            'gin': HF.decimate2_bwd(T.P(gy), DECIMATE)}

  def verify(out):
    bits = lambda t: t.view(torch.int32)
    assert torch.equal(bits(out['gdisp']), bits(out['autograd_d'])) and torch.equal(bits(out['gconf']), bits(out['autograd_c']))
    winner, _ = R.decode_keys(out['keys'])
    assert torch.equal(bits(out['gconf'][:, 0]), bits(gout[:, 1]))
    assert torch.equal(bits(out['gconf'][:, 3:]), bits(C.winners_scatter(winner, gout[:, 7::2])))
    ref = C.handoff_conf_gradient(conf, winner, gout[:, 1::2])
    T.close(out, 'gconf', ref, 1e-5)  # (the kernel's own bound is that of tests/test_gpu_conf_grad.py; here: the right numbers at all)
    assert zeroed <= 0.01
    h = C.head_reference(lg, gp, gc, size)
    T.close(out, 'gl', h['g_pred'] + h['g_conf'], 1e-4)
    assert torch.equal(bits(out['gin']), bits(C.decimate2_bwd(gy, DECIMATE)))

  return run, verify


_FIRST = len(T.CASES)
T.case('conf_grad', list(NEW_ENTRIES), b_conf_grad)
CASES = T.CASES[_FIRST:_FIRST + 1]


def test_the_case_declares_the_three_entries():
  """CPU tier.  Together with the rest of the table it covers the launching ABI (the ledger of tests/test_guard_bands_host.py)."""
  assert set().union(*[c.entries for c in CASES]) == set(NEW_ENTRIES)
  assert all(c in T.CASES for c in CASES) and len({c.id for c in T.CASES}) == len(T.CASES)
  import test_guard_bands_host as G
  assert set(NEW_ENTRIES) <= G.launching_entries() and set(NEW_ENTRIES) <= G._declared_entries()


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
def test_guarded_conf_grad(c, monkeypatch, stop_at_a_gpu_fault):
  rec, stats = T.run_case(c, monkeypatch)
  assert c.entries, 'every case declares the entries it is there to launch'
  missing = sorted(c.entries - set(rec.launched))
  assert not missing, 'declared but not launched: %s (launched: %s)' % (missing, sorted(rec.launched))
  assert set(rec.launched) <= set(NEW_ENTRIES) | set(FORWARDS), sorted(rec.launched)
  assert rec.launched['mode_multiview_handoff_bwd_full'] >= 4  # two calls under each fill
  T.STATS['allocations'] += sum(stats['allocations'])
  T.STATS['launches'] += sum(rec.launched.values())
  T.STATS['cases'] += 1
  print('  %d guarded allocations, %d launching calls' % (sum(stats['allocations']), sum(rec.launched.values())))
  print('LAUNCHED %s %s' % (c.id, ' '.join(sorted(rec.launched))))
