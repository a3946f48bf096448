"""3D60 ingest, CPU tier: the numpy restatement of the kernels' arithmetic (tests/erp_ref.py) against the reference's own output
(tests/golden/erp3d60.npz, made by tests/golden/make_golden_3d60.py), the grid builder, the host Dataset3D60Disparity on a list file,
the host-side argument checks of the two C-ABI entries (no launch), and the cv2-less error path.

Images, byte images and the float re-projection of the depth are compared bit for bit.  Disparities are compared by their NaN set and
within DISP_TOL: the fixture holds what numpy 2 computes (float32 products of two arrays, float64 after the masked array meets a
Python scalar); the kernel and erp_ref evaluate the sine rule with those types and round to float32 once, on the store, and asin is
not correctly rounded anywhere."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import erp_ref as R
import mode_hip
from dataloader import dataset3D60Loader as L
from utils import geometry as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'erp3d60.npz')
CASES = {'a': ((32, 64), (64, 32)), 'b': ((30, 61), (48, 20))}  # tag -> ERP (He, We), Cassini (H, W)
PAIRS = ('lr', 'ud', 'ur')
VIEWS = {'lr': ('l', 'r'), 'ud': ('u', 'l'), 'ur': ('u', 'r')}  # the left and right view of a pair
DISP_TOL = 1e-3  # px: the project's parity bound for disparities


@pytest.fixture(scope='module')
def z():
  with np.load(GOLDEN, allow_pickle=False) as f:
    return {k: f[k] for k in f.files}


def bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_disp(got, want, what):
  """The fixture's NaN positions exactly, finite values within DISP_TOL."""
  got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
  assert got.shape == want.shape, (what, got.shape, want.shape)
  assert np.array_equal(np.isnan(got), np.isnan(want)), '%s: NaN positions differ' % what
  assert np.isnan(want).any() and not np.isnan(want).all(), what
  err = float(np.nanmax(np.abs(got - want)))
  print('  %s: max |disp - fixture| = %.3e px' % (what, err))
  assert err <= DISP_TOL, (what, err)
  return err


@pytest.mark.parametrize('pair', PAIRS)
@pytest.mark.parametrize('tag', sorted(CASES))
def test_erp_ref_equals_the_reference_bit_for_bit(z, tag, pair):
  key = '%s/%s/' % (tag, pair)
  l, r = VIEWS[pair]
  grid = z[key + 'grid']
  rgb_l, rgb_r = z['%s/rgb_%s' % (tag, l)], z['%s/rgb_%s' % (tag, r)]
  f32 = R.bilinear(rgb_l, grid)
  assert np.array_equal(bits(f32), bits(z[key + 'left_f32']))
  left, right = R.cassini_u8(rgb_l, grid), R.cassini_u8(rgb_r, grid)
  assert np.array_equal(left, z[key + 'left_u8']) and np.array_equal(right, z[key + 'right_u8'])
  # the trap this fixture is there for: inside the re-projected flat block of 255 the exact sum lands just below 255 at some pixels
  # and truncates to 254 -- and only there; a restatement that is merely close in float cannot reproduce the set
  flat = R.bilinear((rgb_l != 255).any(-1).astype(np.float32), grid) == 0.0  # every corner that carries weight lies inside the block
  assert flat.sum() > 20 and (z[key + 'left_u8'][flat] == 254).any() and (z[key + 'left_u8'][flat] >= 254).all()
  assert np.array_equal(left[flat], z[key + 'left_u8'][flat])
  for name, u8 in (('leftImg', left), ('rightImg', right), ('leftImg_flip', right[:, ::-1]), ('rightImg_flip', left[:, ::-1])):
    assert torch.equal(R.norm_lookup(u8), torch.from_numpy(z[key + name])), name
  for view, name in ((l, 'depth_left_f32'), (r, 'depth_right_f32')):
    assert np.array_equal(bits(R.bilinear(z['%s/depth_%s' % (tag, view)], grid)), bits(z[key + name])), name
  assert_disp(R.disparity(z['%s/depth_%s' % (tag, l)], grid)[0], z[key + 'dispMap'][0], 'dispMap')
  assert_disp(R.disparity(z['%s/depth_%s' % (tag, r)], grid, mirror=True)[0], z[key + 'dispMap_flip'][0], 'dispMap_flip')


def test_erp_ref_equals_torch_on_the_hand_made_grid():
  """The grid tests/test_gpu_erp3d60.py feeds the raw entry: border clamp, last row and column, one ulp inside the corners."""
  import torch.nn.functional as F
  u8, depth, grid = R.hand_made()
  g = torch.from_numpy(grid)[None]
  for img in (u8[0, 0], u8[1, 1]):
    want = F.grid_sample(torch.from_numpy(img).float().permute(2, 0, 1)[None], g, mode='bilinear', padding_mode='border', align_corners=True)
    assert np.array_equal(bits(R.bilinear(img, grid)), bits(want[0].permute(1, 2, 0).numpy()))
  for d in depth:
    want = F.grid_sample(torch.from_numpy(d)[None, None], g, mode='bilinear', padding_mode='border', align_corners=True)
    assert np.array_equal(bits(R.bilinear(d, grid)), bits(want[0, 0].numpy()))


def test_the_fixture_exercises_the_threshold_and_the_mask(z):
  for tag in CASES:
    d = z[tag + '/lr/depth_left_f32']
    assert (d > 20).any() and (d <= 0).any() and (d < 0.1).any() and ((d > 0) & (d <= 20)).any()
    assert int(np.isnan(z[tag + '/lr/dispMap']).sum()) == int(((d > 20) | (d <= 0)).sum())


@pytest.mark.parametrize('pair', PAIRS)
@pytest.mark.parametrize('tag', sorted(CASES))
def test_erp2rect_grid_equals_the_grid_the_reference_sampled_with(z, tag, pair):
  H, W = CASES[tag][1]
  grid = G.erp2rect_grid(G.pair_rotation(pair), H, W)
  assert grid.dtype == np.float32 and grid.shape == (H, W, 2) and not grid.flags.writeable
  assert np.array_equal(bits(grid), bits(z['%s/%s/grid' % (tag, pair)]))
  assert G.erp2rect_grid(G.pair_rotation(pair), H, W) is grid  # cached


def test_rotations():
  assert np.array_equal(G.pair_rotation('lr'), np.eye(3, dtype=np.float32)) and G.pair_rotation('ud').dtype == np.float32
  assert np.allclose(G.pair_rotation('ud'), [[0, 1, 0], [-1, 0, 0], [0, 0, 1]], atol=1e-7)
  s = np.sqrt(0.5)
  assert np.allclose(G.pair_rotation('ur'), [[s, s, 0], [-s, s, 0], [0, 0, 1]], atol=1e-7)
  assert np.allclose(G.rodrigues(np.array([0.3, -0.2, 0.5])) @ G.rodrigues(np.array([-0.3, 0.2, -0.5])), np.eye(3), atol=1e-12)
  with pytest.raises(ValueError):
    G.pair_rotation('all')


def _write_tree(z, tag, root, suffix):
  """The fixture's sample as the first of three list-file lines; lines 1 and 2 name files of their own."""
  lines = []
  for i, sub in enumerate(('s0', 's1', 's2')):
    for view, d in (('l', 'Center_Left_Down'), ('r', 'Right'), ('u', 'Up')):
      os.makedirs(os.path.join(root, d, sub), exist_ok=True)
      rgb, depth = z['%s/rgb_%s' % (tag, view)], z['%s/depth_%s' % (tag, view)]
      if i:  # other content: a wrong index cannot pass
        rgb, depth = np.roll(rgb, 3 * i, axis=1), np.roll(depth, 3 * i, axis=1)
      Image.fromarray(rgb).save(os.path.join(root, d, sub, 'color.png'))
      with open(os.path.join(root, d, sub, 'depth' + suffix), 'wb') as f:
        np.save(f, depth)
    lines.append(' '.join(['./%s/color.png' % sub] * 3 + ['./%s/depth%s' % (sub, suffix)] * 3))
  path = os.path.join(root, 'list.txt')
  with open(path, 'w') as f:
    f.write('\n'.join(lines) + '\n')
  return path


@pytest.mark.parametrize('tag', sorted(CASES))
def test_host_loader_equals_the_reference_on_a_list_file(z, tag, tmp_path):
  root = str(tmp_path)
  listfile = _write_tree(z, tag, root, '.npy')
  H, W = CASES[tag][1]
  for pair in PAIRS:
    ds = L.Dataset3D60Disparity(listfile, rootDir=root, curStage='training', shape=(H, W), pair=pair, flip=True, maxDepth=20.0)
    assert len(ds) == 3
    item = ds[0]
    key = '%s/%s/' % (tag, pair)
    assert sorted(item) == sorted(['leftImg', 'rightImg', 'dispMap', 'leftImg_flip', 'rightImg_flip', 'dispMap_flip', 'leftNames', 'rightNames'])
    for k in ('leftImg', 'rightImg', 'leftImg_flip', 'rightImg_flip'):
      assert torch.equal(item[k], torch.from_numpy(z[key + k])), (pair, k)
    for k in ('dispMap', 'dispMap_flip'):  # the same numpy expressions as the reference's: the same values, NaN included
      assert item[k].shape == (1, H, W) and np.array_equal(item[k].numpy(), z[key + k], equal_nan=True), (pair, k)
    l, r = {'lr': ('Center_Left_Down', 'Right'), 'ud': ('Up', 'Center_Left_Down'), 'ur': ('Up', 'Right')}[pair]
    assert item['leftNames'] == os.path.join(root, l + '/', 's0/color.png') and item['rightNames'] == os.path.join(root, r + '/', 's0/color.png')
    other = ds[2]
    assert other['leftNames'].endswith('s2/color.png') and not torch.equal(other['leftImg'], item['leftImg'])
  # device_ingest=True: the decoded inputs and the pair name, nothing computed
  ds = L.Dataset3D60Disparity(listfile, rootDir=root, shape=(H, W), pair='ud', device_ingest=True)
  raw = ds[0]
  assert raw['pair'] == 'ud' and raw['pairs_u8'].dtype == torch.uint8 and raw['pairs_u8'].shape == (2,) + CASES[tag][0] + (3,)
  assert np.array_equal(raw['pairs_u8'][0].numpy(), z[tag + '/rgb_u']) and np.array_equal(raw['pairs_u8'][1].numpy(), z[tag + '/rgb_l'])
  assert np.array_equal(raw['depth_left'].numpy(), z[tag + '/depth_u']) and np.array_equal(raw['depth_right'].numpy(), z[tag + '/depth_l'])
  batch = torch.utils.data.DataLoader(ds, batch_size=3)
  b = next(iter(batch))
  assert b['pairs_u8'].shape == (3, 2) + CASES[tag][0] + (3,) and list(b['pair']) == ['ud'] * 3 and b['depth_left'].shape == (3,) + CASES[tag][0]
  # crop: a window of half the size out of the same item; the host path only
  crop = L.Dataset3D60Disparity(listfile, rootDir=root, shape=(H, W), pair='lr', crop=True)[0]
  assert sorted(crop) == ['dispMap', 'leftImg', 'leftNames', 'rightImg'] and crop['leftImg'].shape == (3, H // 2, W // 2)
  assert crop['dispMap'].shape == (1, H // 2, W // 2)
  with pytest.raises(ValueError, match='host-path'):
    L.Dataset3D60Disparity(listfile, rootDir=root, shape=(H, W), crop=True, device_ingest=True)
  drawn = {L.Dataset3D60Disparity(listfile, rootDir=root, shape=(H, W), pair='all')._draw_pair() for _ in range(64)}
  assert drawn <= {'lr', 'ud', 'ur'} and len(drawn) > 1


def test_exr_without_cv2_is_an_error_that_says_so(z, tmp_path, monkeypatch):
  root = str(tmp_path)
  listfile = _write_tree(z, 'a', root, '.exr')
  ds = L.Dataset3D60Disparity(listfile, rootDir=root, shape=(64, 32), pair='lr')  # constructing reads nothing
  monkeypatch.setitem(sys.modules, 'cv2', None)  # `import cv2` raises ImportError, whether or not the machine has it
  with pytest.raises(RuntimeError, match='needs cv2'):
    ds[0]
  # an injected loader takes its place
  ds = L.Dataset3D60Disparity(listfile, rootDir=root, shape=(64, 32), pair='lr', depthloader=lambda p: np.load(p))
  assert torch.equal(ds[0]['leftImg'], torch.from_numpy(z['a/lr/leftImg']))


def test_argument_validation_without_gpu():
  """Both entries refuse bad arguments on the host, before any launch, with a message."""
  lib = mode_hip.lib()
  null, p16, p4 = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(4100)

  def pairs(**kw):
    a = dict(pairs=p16, grid=p16, lut=p16, N=2, He=30, We=61, H=48, W=20, G=1, left=p16, right=p16, lf=p16, rf=p16, u8=p16)
    a.update(kw)
    return lib.mode_erp_pairs_u8_cassini(a['pairs'], a['grid'], a['lut'], a['N'], a['He'], a['We'], a['H'], a['W'], a['G'], a['left'],
                                         a['right'], a['lf'], a['rf'], a['u8'], null)

  def depth(**kw):
    a = dict(depth=p16, grid=p16, cols=p16, N=2, He=30, We=61, H=48, W=20, G=2, disp=p16, dc=null)
    a.update(kw)
    return lib.mode_erp_depth_disp(a['depth'], a['grid'], a['cols'], a['N'], a['He'], a['We'], a['H'], a['W'], a['G'], 0.26, 20.0, 0, a['disp'],
                                   a['dc'], null)

  for call, bad, msg in (
      (pairs, dict(pairs=null), b'null pointer'), (pairs, dict(grid=null), b'null pointer'), (pairs, dict(lut=null), b'null pointer'),
      (pairs, dict(left=null), b'null pointer'), (pairs, dict(right=null), b'null pointer'), (pairs, dict(lf=null), b'both or neither'),
      (pairs, dict(grid=p4), b'aligned'), (pairs, dict(left=p4), b'aligned'), (pairs, dict(rf=p4), b'aligned'),
      (pairs, dict(u8=ctypes.c_void_p(4098)), b'aligned'), (pairs, dict(G=3), b'must be 1 or N'), (pairs, dict(G=0), b'must be 1 or N'),
      (pairs, dict(He=1), b'ERP size'), (pairs, dict(We=1), b'ERP size'), (pairs, dict(W=18), b'multiple of 4'), (pairs, dict(W=0), b'bad size'),
      (pairs, dict(H=0), b'bad size'), (pairs, dict(N=-1), b'bad size'), (pairs, dict(N=8, G=8, H=16384, W=16384), b'too large'),
      (pairs, dict(He=20000, We=20000), b'too large'),
      (depth, dict(depth=null), b'null pointer'), (depth, dict(grid=null), b'null pointer'), (depth, dict(cols=null), b'null pointer'),
      (depth, dict(disp=null), b'null pointer'), (depth, dict(grid=p4), b'aligned'), (depth, dict(cols=p4), b'aligned'),
      (depth, dict(disp=p4), b'aligned'), (depth, dict(dc=p4), b'aligned'), (depth, dict(G=3), b'must be 1 or N'), (depth, dict(He=1), b'ERP size'),
      (depth, dict(W=22), b'multiple of 4'), (depth, dict(N=-2), b'bad size'), (depth, dict(N=9, G=9, H=16384, W=16384), b'too large'),
  ):
    rc = call(**bad)
    assert rc == -1 and msg in lib.mode_last_error(), (call.__name__, bad, rc, lib.mode_last_error())
  # N = 0 is a no-op, whatever the pointers
  assert pairs(N=0, pairs=null, left=null) == 0 and depth(N=0, G=0, depth=null, disp=null) == 0


def test_python_wrappers_refuse_what_is_not_on_a_gpu():
  from dataloader import gpu_ingest
  with pytest.raises(NotImplementedError):
    gpu_ingest.erp_pairs_gpu(torch.zeros(1, 2, 8, 16, 3, dtype=torch.uint8), shape=(16, 8))
  with pytest.raises(ValueError, match='multiple of 4'):
    gpu_ingest.erp_pairs_gpu(torch.zeros(1, 2, 8, 16, 3, dtype=torch.uint8), shape=(16, 6))
  with pytest.raises(ValueError, match='pair names'):
    gpu_ingest.erp_pairs_gpu(torch.zeros(2, 2, 8, 16, 3, dtype=torch.uint8), pair=['lr'], shape=(16, 8))
