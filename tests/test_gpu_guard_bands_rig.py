"""Guard bands for the three launching entries of the rig hand-off (mode_multiview_rig_handoff, mode_multiview_rig_handoff_bwd,
mode_multiview_rig_handoff_bwd_full): no read or write outside the buffers they were given.

As tests/test_gpu_guard_bands_conf_grad.py and tests/test_gpu_guard_bands_spp.py: the case is registered in the operator table of
tests/test_gpu_guard_bands.py (test_gpu_guard_bands.CASES, through its own case() helper) when this module is imported, so the ledger
of tests/test_guard_bands_host.py sees the entries whenever the suite is collected as a whole.  It runs here through
test_gpu_guard_bands.run_case (declared entries launched, guards intact under both fills, outputs bit-equal between the fills and
finite).

One case: the 16-pair rig of tests/rig_ref.py (every kind, interleaved and repeated; six rotation grids and eight view transforms,
so every table index and every key-plane offset up to the largest the entries take) at (40, 24) -- a width that is no power of two;
960 pixels: a ragged last block -- and F = 2 (plane and key-plane offsets of a second frame).  The disparities, the confidence, the
upstream gradient, the forward's keys and the CSR arrays of the adjoint lists are placed between guards; the rotation grids, the
trig table, the workspace and every output are allocations of the host code, which the guard allocator relocates and fills with a
different pattern in each of the two runs: bit equality between the fills also proves that every element is written."""
import pytest
import torch

import test_gpu_guard_bands as T

import rig_ref as RR
from utils import geometry as HG

RIG_ENTRIES = ('mode_multiview_rig_handoff', 'mode_multiview_rig_handoff_bwd', 'mode_multiview_rig_handoff_bwd_full')
SHAPE = (2, 40, 24)


def _fresh_caches():
  T._fresh_caches()
  HG._adjoint_cache.clear()


def b_rig_handoff(F_, H, W):
  rig = RR.mixed16()
  P = len(rig.pairs)
  disp, conf = RR.inputs(F_, P, H, W, 7 + F_ + H, 'cpu')
  gout = torch.randn(F_, 2 * P, H, W, generator=torch.Generator().manual_seed(11 + F_ + H))
  lists = HG._rig_adjoint(rig, H, W, 'cpu')

  def run():
    _fresh_caches()
    d, c, g = T.P(disp), T.P(conf), T.P(gout)
    out, keys = HG.disp2depth_frames_gpu(d, c, rig=rig, return_keys=True)
    png = HG.disp2depth_frames_gpu(d, c, rig=rig, conf_png=True)
    alone = HG.disp2depth_frames_gpu(d, c, rig=rig, depth_only=True)
    keys = T.P(keys.cpu())
    HG._adjoint_cache[(rig, H, W, str(d.device))] = tuple(T.P(t) for t in lists)
    gdisp = HG.disp2depth_frames_bwd(d, g, keys, rig=rig)
    g_alone = HG.disp2depth_frames_bwd(d, T.P(gout[:, 0::2].contiguous()), keys, rig=rig, depth_only=True)
    gfull, gconf = HG.disp2depth_frames_bwd(d, g, keys, rig=rig, conf_grad=True)
    ld, lc = T.P(disp).requires_grad_(True), T.P(conf).requires_grad_(True)
    through = torch.autograd.grad(HG.disp2depth_frames_gpu(ld, lc, rig=rig, conf_grad=True), (ld, lc), g)
    return {'out': out, 'png': png, 'alone': alone, 'keys': keys, 'gdisp': gdisp, 'g_alone': g_alone, 'gfull': gfull, 'gconf': gconf,
            'autograd_d': through[0], 'autograd_c': through[1]}

  def verify(out):
    bits = lambda t: t.view(torch.int32)
    d, c = disp.to(T.DEV), conf.to(T.DEV)
    want = RR.single_calls(d, c, rig).cpu()  # (the right numbers at all: the P single calls, outside the guarded runs)
    assert torch.equal(bits(out['out']), bits(want)) and torch.equal(bits(out['alone']), bits(want[:, 0::2]))
    assert torch.equal(bits(out['png'][:, 0::2]), bits(want[:, 0::2]))
    assert torch.equal(bits(out['png'][:, 1::2]), bits(torch.from_numpy(HG.conf_png_np(want[:, 1::2].numpy()))))
    for k in ('g_alone', 'gfull', 'autograd_d'):
      assert torch.equal(bits(out['gdisp']), bits(out[k])), k
    assert torch.equal(bits(out['gconf']), bits(out['autograd_c']))
    _fresh_caches()
    plain = HG.disp2depth_frames_bwd(d, gout.to(T.DEV), out['keys'].to(T.DEV), rig=rig, conf_grad=True)
    assert torch.equal(bits(plain[0].cpu()), bits(out['gdisp'])) and torch.equal(bits(plain[1].cpu()), bits(out['gconf']))
    assert bool((out['gdisp'] != 0).any()) and bool((out['gconf'] != 0).any())

  return run, verify


_FIRST = len(T.CASES)
T.case('multiview_rig_handoff', list(RIG_ENTRIES), b_rig_handoff, SHAPE)
CASES = T.CASES[_FIRST:_FIRST + 1]


def test_the_case_declares_the_three_entries():
  """CPU tier.  Together with the rest of the table it covers the launching ABI (the ledger of tests/test_guard_bands_host.py)."""
  assert set().union(*[c.entries for c in CASES]) == set(RIG_ENTRIES)
  assert all(c in T.CASES for c in CASES) and len({c.id for c in T.CASES}) == len(T.CASES)
  import test_guard_bands_host as G
  assert set(RIG_ENTRIES) <= G.launching_entries() and set(RIG_ENTRIES) <= G._declared_entries()


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
def test_guarded_rig_handoff(c, monkeypatch, stop_at_a_gpu_fault):
  rec, stats = T.run_case(c, monkeypatch)
  assert c.entries, 'every case declares the entries it is there to launch'
  missing = sorted(c.entries - set(rec.launched))
  assert not missing, 'declared but not launched: %s (launched: %s)' % (missing, sorted(rec.launched))
  assert set(rec.launched) <= set(RIG_ENTRIES), sorted(rec.launched)
  assert rec.launched['mode_multiview_rig_handoff'] >= 8 and rec.launched['mode_multiview_rig_handoff_bwd_full'] >= 4
  T.STATS['allocations'] += sum(stats['allocations'])
  T.STATS['launches'] += sum(rec.launched.values())
  T.STATS['cases'] += 1
  print('  %d guarded allocations, %d launching calls' % (sum(stats['allocations']), sum(rec.launched.values())))
  print('LAUNCHED %s %s' % (c.id, ' '.join(sorted(rec.launched))))
