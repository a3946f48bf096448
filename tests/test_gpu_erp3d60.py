"""3D60 ingest, GPU tier: mode_erp_pairs_u8_cassini and mode_erp_depth_disp against the reference's own output
(tests/golden/erp3d60.npz) and the numpy restatement of their arithmetic (tests/erp_ref.py).

Images are compared with torch.equal: the re-projection has the bits of torch's CPU grid_sample, the rest is a truncation, a table
lookup and a mirror.  The re-projected depth is bit-equal too.  Disparities have exactly the fixture's NaN positions and lie within
1e-3 px of it (the project's parity bound for disparities): asin is the one operation that is not correctly rounded on either side,
and the fixture's values are numpy 2's float64 (tests/golden/make_golden_3d60.py).  The largest difference seen is printed."""
import os

import numpy as np
import pytest
import torch

import erp_ref as R
import recipe
from dataloader import dataset3D60Loader as L
from dataloader import gpu_ingest
from mode_hip import functional as HF
from test_erp3d60_host import CASES, DISP_TOL, PAIRS, VIEWS, _write_tree, assert_disp, bits

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'erp3d60.npz')
IMAGES = ('leftImg', 'rightImg', 'leftImg_flip', 'rightImg_flip')


@pytest.fixture(scope='module')
def z():
  with np.load(GOLDEN, allow_pickle=False) as f:
    return {k: f[k] for k in f.files}


def _batch(z, tag, pairs):
  """The fixture's sample once per pair name: (pairs_u8 (N, 2, He, We, 3), depth_left, depth_right (N, He, We)) on the device."""
  u8 = np.stack([np.stack((z['%s/rgb_%s' % (tag, VIEWS[p][0])], z['%s/rgb_%s' % (tag, VIEWS[p][1])])) for p in pairs])
  dl = np.stack([z['%s/depth_%s' % (tag, VIEWS[p][0])] for p in pairs])
  dr = np.stack([z['%s/depth_%s' % (tag, VIEWS[p][1])] for p in pairs])
  return torch.from_numpy(u8).to(DEV), torch.from_numpy(dl).to(DEV), torch.from_numpy(dr).to(DEV)


def _check(out, z, tag, pairs):
  worst = 0.0
  for n, p in enumerate(pairs):
    key = '%s/%s/' % (tag, p)
    for k in IMAGES:
      assert torch.equal(out[k][n].cpu(), torch.from_numpy(z[key + k])), (tag, p, n, k)
    assert torch.equal(out['cassini_u8'][n, 0].cpu(), torch.from_numpy(z[key + 'left_u8'])), (tag, p, n)
    assert torch.equal(out['cassini_u8'][n, 1].cpu(), torch.from_numpy(z[key + 'right_u8'])), (tag, p, n)
    for k in ('dispMap', 'dispMap_flip'):
      assert out[k].dtype == torch.float32
      worst = max(worst, assert_disp(out[k][n].cpu().numpy(), z[key + k], '%s %s %s' % (tag, p, k)))
  return worst


@pytest.mark.parametrize('tag', sorted(CASES))
def test_ingest_is_the_reference_byte_for_byte(z, tag):
  H, W = CASES[tag][1]
  worst = 0.0
  for p in PAIRS:  # N = 1, one grid
    u8, dl, dr = _batch(z, tag, (p,))
    out = gpu_ingest.erp_pairs_gpu(u8, dl, dr, pair=p, shape=(H, W), return_u8=True)
    assert sorted(out) == sorted(IMAGES + ('dispMap', 'dispMap_flip', 'cassini_u8')) and out['leftImg'].shape == (1, 3, H, W)
    assert out['dispMap'].shape == (1, 1, H, W)
    worst = max(worst, _check(out, z, tag, (p,)))
    plain = gpu_ingest.erp_pairs_gpu(u8, dl, pair=p, shape=(H, W), flip=False)
    assert sorted(plain) == ['dispMap', 'leftImg', 'rightImg']
    assert all(torch.equal(plain[k].view(torch.int32), out[k].view(torch.int32)) for k in plain)  # (bits: the disparity holds NaN)
    assert sorted(gpu_ingest.erp_pairs_gpu(u8, pair=p, shape=(H, W))) == sorted(IMAGES)  # no depth: no disparity keys
  mixed = ('ud', 'lr', 'ur')  # N = 3, a grid per sample (G = N)
  u8, dl, dr = _batch(z, tag, mixed)
  out = gpu_ingest.erp_pairs_gpu(u8, dl, dr, pair=list(mixed), shape=(H, W), return_u8=True)
  worst = max(worst, _check(out, z, tag, mixed))
  same = ('ur',) * 3  # N = 3 on one grid (G = 1): every sample walks the same taps
  u8, dl, dr = _batch(z, tag, same)
  worst = max(worst, _check(gpu_ingest.erp_pairs_gpu(u8, dl, dr, pair='ur', shape=(H, W), return_u8=True), z, tag, same))
  empty = gpu_ingest.erp_pairs_gpu(u8[:0], dl[:0], dr[:0], pair='lr', shape=(H, W))  # N = 0: nothing launched
  assert empty['leftImg'].shape == (0, 3, H, W) and empty['dispMap_flip'].shape == (0, 1, H, W)
  print('largest |disp - fixture| on %s: %.3e px (bound %.0e)' % (tag, worst, DISP_TOL))


@pytest.mark.parametrize('tag', sorted(CASES))
def test_depth_cassini_is_bit_equal_and_the_mirror_comes_before_the_sine_rule(z, tag):
  H, W = CASES[tag][1]
  for p in PAIRS:
    key = '%s/%s/' % (tag, p)
    grid = torch.from_numpy(z[key + 'grid'])[None].to(DEV)
    cols = torch.from_numpy(L.disp_cols(W)).to(DEV)
    for view, name, mirror in ((VIEWS[p][0], 'depth_left_f32', False), (VIEWS[p][1], 'depth_right_f32', True)):
      depth = torch.from_numpy(z['%s/depth_%s' % (tag, view)])[None].to(DEV)
      disp, dc = HF.erp_depth_disp(depth, grid, cols, 0.26, 20.0, mirror=mirror, return_depth=True)
      want = z[key + name].copy()
      want = np.ascontiguousarray(want[:, ::-1]) if mirror else want
      want[want > 20.0] = 0
      assert np.array_equal(bits(dc[0].cpu().numpy()), bits(want)), (tag, p, name)
      ref_disp, ref_dc = R.disparity(z['%s/depth_%s' % (tag, view)], z[key + 'grid'], mirror=mirror)
      assert np.array_equal(bits(ref_dc), bits(want))
      assert_disp(disp[0, 0].cpu().numpy(), ref_disp, '%s %s %s against erp_ref' % (tag, p, name))
      assert torch.equal(HF.erp_depth_disp(depth, grid, cols, 0.26, 20.0, mirror=mirror).isnan(), disp.isnan())


def test_hand_made_grid_through_the_raw_entry_equals_erp_ref():
  """-1, +1, values beyond both (the border clamp), points exactly on the last row and column, on an odd-sized source."""
  u8, depth, grid = R.hand_made()
  N, W = u8.shape[0], grid.shape[1]
  d_u8, d_grid = torch.from_numpy(u8).to(DEV), torch.from_numpy(grid)[None].to(DEV)
  lut = gpu_ingest._norm_lut(torch.device(DEV))
  left, right, lf, rf, c8 = HF.erp_pairs_u8_cassini(d_u8, d_grid, lut, flip=True, return_u8=True)
  for n in range(N):
    wl, wr = R.cassini_u8(u8[n, 0], grid), R.cassini_u8(u8[n, 1], grid)
    assert np.array_equal(c8[n, 0].cpu().numpy(), wl) and np.array_equal(c8[n, 1].cpu().numpy(), wr), n
    assert torch.equal(left[n].cpu(), R.norm_lookup(wl)) and torch.equal(right[n].cpu(), R.norm_lookup(wr))
    assert torch.equal(lf[n].cpu(), R.norm_lookup(wr[:, ::-1])) and torch.equal(rf[n].cpu(), R.norm_lookup(wl[:, ::-1]))
  cols = torch.from_numpy(L.disp_cols(W)).to(DEV)
  for mirror in (False, True):
    disp, dc = HF.erp_depth_disp(torch.from_numpy(depth).to(DEV), d_grid, cols, 0.26, 20.0, mirror=mirror, return_depth=True)
    for n in range(N):
      ref_disp, ref_dc = R.disparity(depth[n], grid, mirror=mirror)
      assert np.array_equal(bits(dc[n].cpu().numpy()), bits(ref_dc)), (n, mirror)
      assert np.isnan(ref_disp).any()
      assert_disp(disp[n, 0].cpu().numpy(), ref_disp, 'hand-made grid, sample %d, mirror %d' % (n, mirror))


def _loaders(z, tag, root, pair):
  listfile = _write_tree(z, tag, root, '.npy')
  H, W = CASES[tag][1]
  host = L.Dataset3D60Disparity(listfile, rootDir=root, shape=(H, W), pair=pair)
  dev = L.Dataset3D60Disparity(listfile, rootDir=root, shape=(H, W), pair=pair, device_ingest=True)
  return host, dev


@pytest.mark.parametrize('tag', sorted(CASES))
def test_device_loader_equals_host_loader(z, tag, tmp_path):
  H, W = CASES[tag][1]
  for pair in PAIRS:
    host, dev = _loaders(z, tag, str(tmp_path), pair)
    want = next(iter(torch.utils.data.DataLoader(host, batch_size=3)))
    b = next(iter(torch.utils.data.DataLoader(dev, batch_size=3)))
    got = gpu_ingest.erp_pairs_gpu(b['pairs_u8'].to(DEV), b['depth_left'].to(DEV), b['depth_right'].to(DEV), pair=b['pair'], shape=(H, W))
    for k in IMAGES:
      assert torch.equal(got[k].cpu(), want[k]), (pair, k)
    for k in ('dispMap', 'dispMap_flip'):
      assert_disp(got[k].cpu().numpy(), want[k].numpy(), '%s %s %s' % (tag, pair, k))


def test_end_to_end_at_64_by_32(z, tmp_path):
  import models
  from utils import evaluation
  H, W, maxdisp = 64, 32, 16
  host, dev = _loaders(z, 'a', str(tmp_path), 'lr')
  want = next(iter(torch.utils.data.DataLoader(host, batch_size=2)))
  b = next(iter(torch.utils.data.DataLoader(dev, batch_size=2)))
  got = gpu_ingest.erp_pairs_gpu(b['pairs_u8'].to(DEV), b['depth_left'].to(DEV), b['depth_right'].to(DEV), pair=b['pair'], shape=(H, W))
  net = models.ModeDisparity(maxdisp, 'Sphere', H, W, 'Cassini').to(DEV)
  net.load_state_dict(recipe.recipe_state_wc(recipe.load_manifest(), 100))
  net.eval()
  with torch.no_grad():
    a = net(got['leftImg'], got['rightImg'])
    c = net(want['leftImg'].to(DEV), want['rightImg'].to(DEV))
  assert torch.equal(a, c) and bool(torch.isfinite(a).all())
  gt = got['dispMap']
  assert bool(gt.isnan().any())
  mask = (gt == gt) & (gt > 0)
  rows = evaluation.disparity_metrics(a, gt, mask)
  assert len(rows) == 6 and all(np.isfinite(float(v)) for v in rows), rows
  net.train()
  loss, preds = net.forward_loss(got['leftImg'], got['rightImg'], gt)  # mode_smooth_l1_masked masks the NaN ground truth
  loss.backward()
  torch.cuda.synchronize()
  assert np.isfinite(float(loss)) and all(bool(torch.isfinite(p.grad).all()) for p in net.parameters() if p.grad is not None)


def test_ingest_replays_from_a_captured_graph(z):
  """Grids, the column table and the normalisation table are uploaded on the first eager call: after it the call captures."""
  H, W = CASES['b'][1]
  pairs = ['ud', 'lr', 'ur']
  first, second = _batch(z, 'b', pairs), _batch(z, 'b', pairs[::-1])
  static = [t.clone() for t in first]
  eager = gpu_ingest.erp_pairs_gpu(*static, pair=pairs, shape=(H, W))
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    out = gpu_ingest.erp_pairs_gpu(*static, pair=pairs, shape=(H, W))
  for batch in (first, second):
    for s, t in zip(static, batch):
      s.copy_(t)
    want = gpu_ingest.erp_pairs_gpu(*batch, pair=pairs, shape=(H, W))
    graph.replay()
    torch.cuda.synchronize()
    once = {k: v.clone() for k, v in out.items()}
    graph.replay()  # and again on the same inputs: identical bits
    torch.cuda.synchronize()
    for k in want:
      assert torch.equal(out[k].view(torch.int32), want[k].view(torch.int32)), k
      assert torch.equal(out[k].view(torch.int32), once[k].view(torch.int32)), k
  assert sorted(eager) == sorted(out)
  del graph
  gpu_ingest._erp_cache.release_graph_pins()
  gpu_ingest._lut_cache.release_graph_pins()
