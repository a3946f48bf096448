"""Guard bands for the 3D60 ingest entries (mode_erp_pairs_u8_cassini, mode_erp_depth_disp): no read or write outside the buffers
they were given.

As tests/test_gpu_guard_bands_ingest.py: the two cases are registered in the operator table of tests/test_gpu_guard_bands.py
(test_gpu_guard_bands.CASES, through its own case() helper) when this module is imported, so the ledger of
tests/test_guard_bands_host.py sees the two entries whenever the suite is collected as a whole.  They run here through
test_gpu_guard_bands.run_case (declared entries launched, guards intact under both fills, outputs bit-equal between the fills and
finite) and verify the values against the reference's own output, tests/golden/erp3d60.npz.

The ingest case is the odd-width fixture (ERP 30 x 61: 3-byte pixels at every byte alignment, the last one ending at the rear guard),
its byte input between the 0x01 / 0x02 guard fills.  The depth case runs the entry with mirror 0 and 1.  A disparity map holds NaN by
design (pixels without a valid depth), so it is returned as its bit pattern: compared between the fills, exempt from the finiteness
check; the re-projected depth next to it is float and finite."""
import os

import numpy as np
import pytest
import torch

import test_gpu_guard_bands as T

from dataloader import dataset3D60Loader as L
from dataloader import gpu_ingest
from mode_hip import functional as HF
from test_erp3d60_host import CASES as SIZES, VIEWS, assert_disp, bits

ERP_ENTRIES = ('mode_erp_pairs_u8_cassini', 'mode_erp_depth_disp')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'erp3d60.npz')
IMAGES = ('leftImg', 'rightImg', 'leftImg_flip', 'rightImg_flip')


def _fresh_caches():
  """Grids, column tables and the normalisation table are cached per device: drop them, so that every run uploads them inside its
  guarded context."""
  T._fresh_caches()
  for c in (gpu_ingest._lut_cache, gpu_ingest._erp_cache):
    c.clear()


def _fixture():
  with np.load(GOLDEN, allow_pickle=False) as f:
    return {k: f[k] for k in f.files}


def b_erp_pairs(tag, *pairs):
  """tests/test_gpu_erp3d60.py: a grid per sample, both flip twins and the 8-bit images; then one shared grid without the twins."""
  z = _fixture()
  H, W = SIZES[tag][1]
  u8 = np.stack([np.stack((z['%s/rgb_%s' % (tag, VIEWS[p][0])], z['%s/rgb_%s' % (tag, VIEWS[p][1])])) for p in pairs])

  def run():
    _fresh_caches()
    out = gpu_ingest.erp_pairs_gpu(T.P(torch.from_numpy(u8)), pair=list(pairs), shape=(H, W), return_u8=True)
    one = gpu_ingest.erp_pairs_gpu(T.P(torch.from_numpy(u8[:1])), pair=pairs[0], shape=(H, W), flip=False)
    out.update({'one_' + k: v for k, v in one.items()})
    return out

  def verify(out):
    for n, p in enumerate(pairs):
      key = '%s/%s/' % (tag, p)
      for k in IMAGES:
        assert torch.equal(out[k][n], torch.from_numpy(z[key + k])), (p, k)
      assert torch.equal(out['cassini_u8'][n, 0], torch.from_numpy(z[key + 'left_u8']))
      assert torch.equal(out['cassini_u8'][n, 1], torch.from_numpy(z[key + 'right_u8']))
    assert torch.equal(out['one_leftImg'][0], out['leftImg'][0]) and torch.equal(out['one_rightImg'][0], out['rightImg'][0])
    assert sorted(k for k in out if k.startswith('one_')) == ['one_leftImg', 'one_rightImg']

  return run, verify


def b_erp_depth(tag, *pairs):
  """mirror 0 on the left views' depth, mirror 1 on the right views' (the flip twin), a grid per sample, with the re-projected depth."""
  z = _fixture()
  H, W = SIZES[tag][1]
  dl = np.stack([z['%s/depth_%s' % (tag, VIEWS[p][0])] for p in pairs])
  dr = np.stack([z['%s/depth_%s' % (tag, VIEWS[p][1])] for p in pairs])
  grid = np.stack([z['%s/%s/grid' % (tag, p)] for p in pairs])

  def run():
    g, cols = T.P(torch.from_numpy(grid)), T.P(torch.from_numpy(L.disp_cols(W)))
    d0, c0 = HF.erp_depth_disp(T.P(torch.from_numpy(dl)), g, cols, 0.26, 20.0, mirror=False, return_depth=True)
    d1, c1 = HF.erp_depth_disp(T.P(torch.from_numpy(dr)), g, cols, 0.26, 20.0, mirror=True, return_depth=True)
    alone = HF.erp_depth_disp(T.P(torch.from_numpy(dl[:1])), T.P(torch.from_numpy(grid[:1])), cols, 0.26, 20.0)
    return {'disp_bits': d0.view(torch.int32), 'flip_bits': d1.view(torch.int32), 'alone_bits': alone.view(torch.int32), 'depth': c0,
            'depth_flip': c1}

  def verify(out):
    for n, p in enumerate(pairs):
      key = '%s/%s/' % (tag, p)
      want, want_f = z[key + 'depth_left_f32'].copy(), np.ascontiguousarray(z[key + 'depth_right_f32'][:, ::-1])
      want[want > 20.0] = 0
      want_f[want_f > 20.0] = 0
      assert np.array_equal(bits(out['depth'][n].numpy()), bits(want)) and np.array_equal(bits(out['depth_flip'][n].numpy()), bits(want_f))
      assert_disp(out['disp_bits'][n, 0].view(torch.float32).numpy(), z[key + 'dispMap'][0], '%s dispMap' % p)
      assert_disp(out['flip_bits'][n, 0].view(torch.float32).numpy(), z[key + 'dispMap_flip'][0], '%s dispMap_flip' % p)
    assert torch.equal(out['alone_bits'][0], out['disp_bits'][0])

  return run, verify


_FIRST = len(T.CASES)
T.case('erp_pairs_u8_cassini', ['mode_erp_pairs_u8_cassini'], b_erp_pairs, ('b', 'ud', 'lr', 'ur'))
T.case('erp_depth_disp', ['mode_erp_depth_disp'], b_erp_depth, ('b', 'ud', 'lr', 'ur'))
CASES = T.CASES[_FIRST:_FIRST + 2]


def test_the_cases_declare_exactly_the_two_erp_entries():
  """CPU tier.  Together with the rest of the table they cover the launching ABI (the ledger of tests/test_guard_bands_host.py)."""
  assert set().union(*[c.entries for c in CASES]) == set(ERP_ENTRIES)
  assert all(c in T.CASES for c in CASES) and len({c.id for c in T.CASES}) == len(T.CASES)
  import test_guard_bands_host as G
  assert set(ERP_ENTRIES) <= G.launching_entries() and set(ERP_ENTRIES) <= G._declared_entries()


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
def test_guarded_erp(c, monkeypatch, stop_at_a_gpu_fault):
  rec, stats = T.run_case(c, monkeypatch)
  assert c.entries, 'every case declares the entries it is there to launch'
  missing = sorted(c.entries - set(rec.launched))
  assert not missing, 'declared but not launched: %s (launched: %s)' % (missing, sorted(rec.launched))
  assert set(rec.launched) <= set(ERP_ENTRIES), sorted(rec.launched)
  T.STATS['allocations'] += sum(stats['allocations'])
  T.STATS['launches'] += sum(rec.launched.values())
  T.STATS['cases'] += 1
  print('  %d guarded allocations, %d launching calls' % (sum(stats['allocations']), sum(rec.launched.values())))
  print('LAUNCHED %s %s' % (c.id, ' '.join(sorted(rec.launched))))
