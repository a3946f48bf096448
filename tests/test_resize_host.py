"""CPU tier of the any-size pair ingest: preprocess.pil_resize_table against Pillow itself, its equality with
pil_half_table, the nearest-neighbour index tables, draw_crop_windows, the argument checks of the two C-ABI entries and the loader's
device_ingest items.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import mode_hip
import resize_ref as R
from dataloader import deep360_loader as L
from dataloader import gpu_ingest as G
from dataloader import preprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('src,dst', R.CASES, ids=['%dx%d-%dx%d' % (s + d) for s, d in R.CASES])
def test_two_passes_with_the_tables_are_pillows_resize(src, dst, kind):
  """Byte for byte Image.resize: the horizontal pass first, stored in 8 bits, a pass of equal size skipped."""
  a = R.image(kind, *src)
  want = R.pil_resize(a, *dst)
  before = list(R.CLIPS)
  got = R.two_pass(a, *dst)
  assert got.shape == want.shape == dst + (3,) and got.dtype == np.uint8
  assert np.array_equal(got, want), int((got != want).sum())
  if kind == 'binary':
    assert R.CLIPS[0] > before[0] and R.CLIPS[1] > before[1]  # sums below 0 and above 255 were clipped: both ends are exercised


def test_tap_counts_are_the_documented_ones():
  ks = {(s, d): (preprocess.pil_resize_table(s[0], d[0])[2].shape[1], preprocess.pil_resize_table(s[1], d[1])[2].shape[1]) for s, d in R.CASES}
  assert ks[((64, 32), (32, 16))] == (9, 9) and ks[((64, 32), (128, 64))] == (5, 5) and ks[((64, 32), (16, 8))] == (17, 17)
  assert ks[((64, 32), (24, 12))] == (13, 13) and ks[((64, 32), (13, 7))] == (21, 21)
  count = lambda n, out: int(preprocess.pil_resize_table(n, out)[1].max())
  assert count(64, 24) == 11 and count(64, 16) == 16 and count(64, 13) == 20 and count(64, 32) == 8 and count(64, 128) == 4
  # every ksize inside the kernels' limit of a factor of 4 fits the 17 taps they take
  assert max(preprocess.pil_resize_table(n, out)[2].shape[1] for n, out in ((64, 16), (16, 64), (37, 10), (9, 36))) == 17


@pytest.mark.parametrize('n', [2, 8, 46, 512])
def test_the_halving_is_pil_half_table_with_a_zero_column(n):
  xmin, count, kk = preprocess.pil_resize_table(n, n // 2)
  hx, hc, hk = preprocess.pil_half_table(n)
  assert kk.shape == (n // 2, 9) and kk.dtype == xmin.dtype == count.dtype == np.int32
  assert np.array_equal(xmin, hx) and np.array_equal(count, hc) and np.array_equal(kk[:, :8], hk) and not kk[:, 8].any()
  assert torch.equal(G.resize_table_rows(n, n // 2)[:, :10], G.half_table_rows(n))


@pytest.mark.parametrize('n,out', [(s[a], d[a]) for s, d in R.CASES for a in (0, 1)] + [(1, 4), (4, 1), (1024, 512), (512, 1024), (1000, 333)])
def test_taps_stay_inside_the_source_and_the_row(n, out):
  xmin, count, kk = preprocess.pil_resize_table(n, out)
  assert xmin.shape == count.shape == (out,) and kk.shape[0] == out
  assert count.min() >= 1 and count.max() <= kk.shape[1] and xmin.min() >= 0 and int((xmin + count).max()) <= n
  assert all(not kk[i, count[i]:].any() for i in range(out))
  assert bool((np.abs(kk.sum(1) - (1 << preprocess.PIL_PRECISION_BITS)) <= kk.shape[1]).all())  # normalised rows, up to the rounding of each tap
  with pytest.raises(ValueError):
    preprocess.pil_resize_table(0, 4)
  with pytest.raises(ValueError):
    preprocess.pil_resize_table(4, 0)


@pytest.mark.parametrize('src,dst', [((64, 32), (32, 16)), ((37, 23), (50, 9)), ((1024, 512), (512, 256)), ((7, 5), (7, 5)), ((10, 6), (33, 17))])
def test_nearest_tables_are_resize_nearests_indices(src, dst):
  rows, cols = preprocess.nearest_index_table(src[0], dst[0]), preprocess.nearest_index_table(src[1], dst[1])
  assert rows.dtype == cols.dtype == np.int32 and rows.shape == (dst[0],) and cols.shape == (dst[1],)
  assert rows.min() >= 0 and rows.max() < src[0] and cols.min() >= 0 and cols.max() < src[1]
  a = np.random.RandomState(7).rand(*src).astype(np.float32)
  assert np.array_equal(a[np.ix_(rows, cols)], L.resize_nearest(a, dst[1], dst[0]))
  if src == dst:
    assert np.array_equal(rows, np.arange(src[0])) and np.array_equal(cols, np.arange(src[1]))


def test_draw_crop_windows_stay_in_range_and_are_reproducible():
  g = lambda s: torch.Generator().manual_seed(s)
  a, b, c = G.draw_crop_windows(500, (40, 30), (16, 8), g(3)), G.draw_crop_windows(500, (40, 30), (16, 8), g(3)), G.draw_crop_windows(500, (40, 30), (16, 8), g(4))
  assert a.dtype == torch.int32 and tuple(a.shape) == (500, 2) and not a.is_cuda
  assert torch.equal(a, b) and not torch.equal(a, c)
  assert int(a[:, 0].min()) == 0 and int(a[:, 0].max()) == 24 and int(a[:, 1].min()) == 0 and int(a[:, 1].max()) == 22  # both ends are reached
  assert len(set(a[:, 0].tolist())) == 25 and len(set(a[:, 1].tolist())) == 23
  d = G.draw_crop_windows(3, (1024, 512))  # the loader's 512 x 256 crop
  assert int(d[:, 0].max()) <= 512 and int(d[:, 1].max()) <= 256 and int(d.min()) >= 0
  assert not G.draw_crop_windows(4, (16, 8), (16, 8)).any()  # a window as large as the image has one place
  assert tuple(G.draw_crop_windows(0, (16, 8), (4, 4)).shape) == (0, 2)
  with pytest.raises(ValueError):
    G.draw_crop_windows(1, (16, 8), (17, 8))
  with pytest.raises(ValueError):
    G.draw_crop_windows(-1, (16, 8), (4, 4))


def test_abi_entries_are_declared_exported_and_bound():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mode_hip.h')).read(), flags=re.S)
  lib = mode_hip.lib()
  names = ('mode_images_u8_resize_pil', 'mode_images_u8_resize_pil_workspace_bytes', 'mode_disp_resize_nearest')
  for name in names:
    assert re.search(r'\b%s\s*\(' % name, src) and hasattr(lib, name) and name in mode_hip.SIGNATURES
  assert [n in mode_hip.LAUNCHING for n in names] == [True, False, True]
  assert all(mode_hip.SIGNATURES[n][1][-1] is ctypes.c_void_p for n in (names[0], names[2]))  # the stream is the last argument
  from mode_hip import functional as HF
  assert HF.RESIZE_MAX_SCALE == mode_hip.CONSTANTS['MODE_RESIZE_MAX_SCALE'] == 4 and HF.RESIZE_MAX_TAPS == preprocess.pil_resize_table(64, 16)[2].shape[1]
  q = lib.mode_images_u8_resize_pil_workspace_bytes
  assert q(3, 64, 32, 24, 12, 24, 12) == 3 * 64 * 12 * 3 and q(3, 64, 32, 24, 12, 5, 7) == 3 * 64 * 7 * 3
  assert q(2, 48, 20, 48, 12, 48, 12) == 0 and q(2, 48, 20, 30, 20, 30, 20) == 0 and q(0, 64, 32, 24, 12, 24, 12) == 0
  code = open(os.path.join(ROOT, 'mode-2022_amd', 'csrc', 'resize.hip')).read()
  assert 'hipMemset' not in code and 'thread_local' not in code and 'atomic' not in re.sub(r'//.*', '', code)


def test_argument_validation_of_the_image_entry_without_gpu():
  """As tests/test_abi.py::test_argument_validation_without_gpu: refused on the host before any launch, with a message."""
  lib = mode_hip.lib()
  null, p = ctypes.c_void_p(0), ctypes.c_void_p(4096)
  f = lib.mode_images_u8_resize_pil
  big = 1 << 30

  def call(images=p, tab_w=p, kw=9, tab_h=p, kh=9, lut=p, windows=null, per=1, split=0, N=2, Hs=64, Ws=32, H=32, W=16, hw=32, ww=16, u8=p, out=p,
           ws=p, nws=big):
    rc = f(images, tab_w, kw, tab_h, kh, lut, windows, per, split, N, Hs, Ws, H, W, hw, ww, u8, out, ws, nws, null)
    return rc, lib.mode_last_error()

  for kw in (dict(images=null), dict(tab_w=null), dict(tab_h=null), dict(u8=null, out=null), dict(lut=null)):
    rc, msg = call(**kw)
    assert rc == -1 and b'null pointer' in msg, kw
  assert b'both outputs' in call(u8=null, out=null)[1]
  # the scale limit: beyond a factor of 4 along an axis, either way, before a pointer is looked at
  for kw in (dict(H=15), dict(W=7), dict(Hs=16, H=65), dict(Ws=8, W=33, ww=16), dict(Hs=64, H=13, hw=13, Ws=32, W=7, ww=7)):
    rc, msg = call(images=null, tab_w=null, tab_h=null, u8=null, out=null, **dict(dict(hw=1, ww=1), **kw))
    assert rc == -2 and b'factor of 4' in msg, kw
  for kw in (dict(H=16, hw=16), dict(W=8, ww=8), dict(Hs=16, H=64), dict(Ws=8, W=32)):  # the limit itself is taken
    rc, msg = call(N=0, **kw)
    assert rc == 0, (kw, msg)
  # a window that does not fit into the resized image
  for kw in (dict(hw=33), dict(ww=17), dict(hw=0), dict(ww=-1)):
    rc, msg = call(**kw)
    assert rc == -1 and b'window' in msg, kw
  for kw in (dict(N=-1), dict(Hs=0), dict(Ws=0), dict(H=0, hw=0), dict(W=-3)):
    rc, msg = call(**kw)
    assert rc == -1 and b'bad size' in msg, kw
  assert b'too large' in call(N=1 << 20, Hs=64, Ws=32)[1] and call(N=1 << 20)[0] == -1  # 3 N Hs Ws >= 2^31
  assert b'too large' in call(N=1, Hs=32768, Ws=16384, H=65536, W=32768, hw=1, ww=1)[1]
  assert b'taps' in call(kw=0)[1] and b'taps' in call(kh=18)[1] and call(kw=0)[0] == -1
  assert b'per window' in call(per=0)[1] and b'per window' in call(per=3, split=1, N=4)[1] and b'per window' in call(split=2)[1]
  assert b'4-byte aligned' in call(tab_w=ctypes.c_void_p(4098))[1] and b'4-byte aligned' in call(windows=ctypes.c_void_p(4097))[1]
  assert b'4-byte aligned' in call(out=ctypes.c_void_p(4102))[1]
  need = lib.mode_images_u8_resize_pil_workspace_bytes(2, 64, 32, 32, 16, 32, 16)
  assert need == 2 * 64 * 16 * 3
  rc, msg = call(nws=need - 1)
  assert rc == -3 and b'workspace' in msg
  assert call(ws=null)[0] == -3
  # N = 0 is a no-op whatever the pointers; a skipped pass needs neither its table nor a workspace to pass the checks
  assert call(images=null, tab_w=null, tab_h=null, lut=null, u8=null, out=null, ws=null, nws=0, N=0)[0] == 0
  assert call(N=0, Hs=48, Ws=20, H=48, W=12, hw=48, ww=12, tab_h=null, kh=0, ws=null, nws=0)[0] == 0


def test_argument_validation_of_the_disparity_entry_without_gpu():
  lib = mode_hip.lib()
  null, p = ctypes.c_void_p(0), ctypes.c_void_p(4096)
  f = lib.mode_disp_resize_nearest

  def call(disp=p, rows=p, cols=p, windows=null, N=2, Hs=64, Ws=32, H=32, W=16, hw=32, ww=16, ratio=0.5, out=p):
    rc = f(disp, rows, cols, windows, N, Hs, Ws, H, W, hw, ww, ratio, out, null)
    return rc, lib.mode_last_error()

  for kw in (dict(disp=null), dict(rows=null), dict(cols=null), dict(out=null)):
    rc, msg = call(**kw)
    assert rc == -1 and b'null pointer' in msg, kw
  for kw in (dict(hw=33), dict(ww=17), dict(hw=0)):
    rc, msg = call(**kw)
    assert rc == -1 and b'window' in msg, kw
  for kw in (dict(N=-1), dict(Hs=0), dict(W=0)):
    rc, msg = call(**kw)
    assert rc == -1 and b'bad size' in msg, kw
  assert b'too large' in call(N=1 << 21)[1] and b'4-byte aligned' in call(rows=ctypes.c_void_p(4098))[1]
  assert call(disp=null, rows=null, cols=null, out=null, N=0)[0] == 0


def test_python_refusals_without_gpu():
  pairs = torch.zeros(1, 2, 8, 4, 3, dtype=torch.uint8)
  with pytest.raises(NotImplementedError):
    G.pairs_u8_gpu(pairs, shape=(4, 2))
  with pytest.raises(NotImplementedError):
    G.resize_u8_gpu(pairs, (4, 2))
  with pytest.raises(ValueError, match='uint8'):
    G.pairs_u8_gpu(pairs.float(), shape=(4, 2))
  with pytest.raises(ValueError, match='uint8'):
    G.resize_u8_gpu(pairs[..., :2], (4, 2))
  with pytest.raises(ValueError, match='factor of 4'):
    G._pil_tables(64, 32, 15, 8, 'cpu')
  with pytest.raises(ValueError, match='outside'):
    G._device_windows(torch.tensor([[0, 3]]), 1, (8, 4), (4, 2), 'cpu', 'x')
  with pytest.raises(ValueError, match='outside'):
    G._device_windows(torch.tensor([[-1, 0]]), 1, (8, 4), (4, 2), 'cpu', 'x')
  with pytest.raises(ValueError, match=r'\(2, 2\)'):
    G._device_windows(torch.tensor([[0, 0]]), 2, (8, 4), (4, 2), 'cpu', 'x')
  ok = G._device_windows(torch.tensor([[4, 2], [0, 0]]), 2, (8, 4), (4, 2), 'cpu', 'x')
  assert ok.dtype == torch.int32 and ok.tolist() == [[4, 2], [0, 0]]
  # the tables are cached per (n, out, device), in a bounded cache
  a, b = G._pil_tables(64, 32, 24, 32, 'cpu'), G._pil_tables(64, 32, 24, 32, 'cpu')
  assert a[0] is None and a[1] is b[1] and tuple(a[1].shape) == (24, 15) and G._resize_cache.maxsize <= 32
  assert G._axis_table('nearest', 64, 24, 'cpu') is G._axis_table('nearest', 64, 24, 'cpu')


def _write_pair(d, name, h, w, seed):
  rng = np.random.RandomState(seed)
  paths = []
  for side in 'ab':
    paths.append(os.path.join(str(d), '%s_%s.png' % (name, side)))
    Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(paths[-1])
  disp = (rng.rand(h, w) * 30).astype(np.float32)
  disp[rng.rand(h, w) < 0.1] = np.nan
  paths.append(os.path.join(str(d), name + '_disp.npz'))
  np.savez(paths[-1], disp)
  return paths


def test_device_ingest_items_are_the_decoded_inputs(tmp_path):
  files = [_write_pair(tmp_path, 'p%d' % i, 16, 8, 20 + i) for i in range(2)]
  lists = [[f[k] for f in files] for k in range(3)]
  ds = L.Deep360DatasetDisparity(*lists, shape=(8, 4), device_ingest=True)
  host = L.Deep360DatasetDisparity(*lists, shape=(16, 8))
  assert len(ds) == 2
  for i in range(2):
    item = ds[i]
    assert set(item) == {'pair_u8', 'disp', 'dispNames'} and item['dispNames'] == lists[2][i]
    assert item['pair_u8'].dtype == torch.uint8 and tuple(item['pair_u8'].shape) == (2, 16, 8, 3) and item['pair_u8'].is_contiguous()
    assert item['disp'].dtype == torch.float32 and tuple(item['disp'].shape) == (16, 8)  # the stored size, whatever `shape` says
    for s, path in enumerate(lists[:2]):
      assert np.array_equal(item['pair_u8'][s].numpy(), np.asarray(Image.open(path[i]).convert('RGB')))
    # the plain transform of those bytes and that map is what the host path returns at the stored size
    h = host[i]
    assert torch.equal(preprocess.get_transform_stage1(augment=False)(item['pair_u8'][0].numpy()), h['leftImg'])
    assert np.array_equal(item['disp'].numpy(), h['dispMap'][0].numpy(), equal_nan=True)
  batch = torch.utils.data.DataLoader(ds, batch_size=2)
  b = next(iter(batch))
  assert tuple(b['pair_u8'].shape) == (2, 2, 16, 8, 3) and tuple(b['disp'].shape) == (2, 16, 8)
  with pytest.raises(ValueError, match='draw_crop_windows'):
    L.Deep360DatasetDisparity(*lists, crop=True, device_ingest=True)
  from dataloader import dataset3D60Loader as D
  with pytest.raises(ValueError, match='crop=True'):  # the 3D60 loader refuses the same combination (before it reads its list)
    D.Dataset3D60Disparity(str(tmp_path / 'none.txt'), rootDir=str(tmp_path), crop=True, device_ingest=True)
