"""GPU tier of the any-size pair ingest (csrc/resize.hip): mode_images_u8_resize_pil against Pillow itself and against the
halving kernel, mode_disp_resize_nearest against the host loader's numpy, the windows, pairs_u8_gpu against the host loader's items,
and a captured-graph replay.  Everything here is bit for bit; the sizes are those of tests/resize_ref.py."""
import functools
import os

import numpy as np
import pytest
import torch
from PIL import Image

import resize_ref as R
from dataloader import deep360_loader as L
from dataloader import gpu_ingest as G
from dataloader import preprocess

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N = 3
GPU_CASES = [c for c in R.CASES if c[1] != (13, 7)]  # (64, 32) -> (13, 7) lies beyond the kernels' limit of a factor of 4
TRANSFORM = preprocess.get_transform_stage1(augment=False)


@functools.lru_cache(maxsize=None)
def _batch(kind, src):
  """N images of one kind and size (read-only)."""
  a = np.stack([R.image(kind, src[0], src[1], seed=n) for n in range(N)])
  a.setflags(write=False)
  return a


@functools.lru_cache(maxsize=None)
def _pillow(kind, src, dst):
  """Pillow's resize of _batch, computed once per case (read-only)."""
  a = np.stack([R.pil_resize(im, *dst) for im in _batch(kind, src)])
  a.setflags(write=False)
  return a


def _disp(n, H, W, seed):
  r = np.random.RandomState(seed)
  d = (r.rand(n, H, W) * 40).astype(np.float32)
  d[r.rand(n, H, W) < 0.15] = np.nan
  d[r.rand(n, H, W) < 0.15] = 0.0
  return d


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('src,dst', GPU_CASES, ids=['%dx%d-%dx%d' % (s + d) for s, d in GPU_CASES])
def test_resize_is_pillows_byte_for_byte(src, dst, kind):
  images = torch.from_numpy(_batch(kind, src).copy()).to(DEV)
  want = _pillow(kind, src, dst)
  got = G.resize_u8_gpu(images, dst)
  assert got.dtype == torch.uint8 and tuple(got.shape) == (N,) + dst + (3,)
  diff = got.cpu().numpy() != want
  assert not diff.any(), '%d of %d bytes differ from PIL.Image.resize' % (int(diff.sum()), diff.size)
  # the fp32 store: the host transform of that resized image
  tab_w, tab_h = G._pil_tables(src[0], src[1], dst[0], dst[1], images.device)
  u8, f32 = G._HF.images_u8_resize_pil(images, dst, tab_w, tab_h, lut=G._norm_lut(images.device), want_f32=True)
  assert torch.equal(u8, got)
  for n in range(N):
    assert torch.equal(f32[n].cpu(), TRANSFORM(want[n])), n
  only = G._HF.images_u8_resize_pil(images, dst, tab_w, tab_h, lut=G._norm_lut(images.device), want_u8=False, want_f32=True)
  assert only[0] is None and torch.equal(only[1], f32)


def test_the_limit_is_refused_and_equal_sizes_return_the_input():
  images = torch.from_numpy(_batch('random', (64, 32)).copy()).to(DEV)
  with pytest.raises(ValueError, match='factor of 4'):
    G.resize_u8_gpu(images, (13, 7))
  assert G.resize_u8_gpu(images, (64, 32)) is images
  frames = images.view(1, 3, 64, 32, 3)  # leading dimensions are kept
  out = torch.empty((1, 3, 24, 12, 3), dtype=torch.uint8, device=DEV)
  assert G.resize_u8_gpu(frames, (24, 12), out=out).data_ptr() == out.data_ptr()
  assert np.array_equal(out[0].cpu().numpy(), _pillow('random', (64, 32), (24, 12)))


def test_the_halving_agrees_with_the_halving_kernel():
  """96 x 80 -> 48 x 40: the general kernel against mode_rgb_half_pil on the same panoramas."""
  frames = torch.from_numpy(np.random.RandomState(9).randint(0, 256, (1, 12, 96, 80, 3)).astype(np.uint8)).to(DEV)
  f32, u8 = G.rgb_half_gpu(frames, return_u8=True)
  panos = frames[:, [0, 1, 10, 11]].contiguous()
  got = G.resize_u8_gpu(panos, (48, 40))
  assert tuple(got.shape) == tuple(u8.shape) == (1, 4, 48, 40, 3) and torch.equal(got, u8)
  tab_w, tab_h = G._pil_tables(96, 80, 48, 40, frames.device)
  planes = G._HF.images_u8_resize_pil(panos.view(4, 96, 80, 3), (48, 40), tab_w, tab_h, lut=G._norm_lut(frames.device), want_u8=False, want_f32=True)[1]
  assert torch.equal(planes.view(1, 12, 48, 40), f32)


WINDOWS = ((0, 0), (24 - 10, 12 - 5), (7, 3))  # of 10 x 5 in the 24 x 12 image: top-left corner, bottom-right corner, interior


@pytest.mark.parametrize('src,dst,crop,windows', [((64, 32), (24, 12), (10, 5), WINDOWS), ((48, 20), (48, 12), (9, 4), ((39, 8), (0, 0), (11, 5))),
                                                  ((20, 48), (12, 48), (4, 9), ((8, 39), (0, 0), (5, 11))), ((16, 8), (16, 8), (5, 3), ((11, 5), (0, 0), (4, 2)))],
                         ids=['both-passes', 'horizontal-only', 'vertical-only', 'copy'])
def test_a_window_is_the_slice_of_the_full_result(src, dst, crop, windows):
  images = torch.from_numpy(_batch('random', src).copy()).to(DEV)
  full = G.resize_u8_gpu(images, dst)
  win = torch.tensor(windows, dtype=torch.int32)
  got = G.resize_u8_gpu(images, dst, windows=win, crop=crop)
  assert tuple(got.shape) == (N,) + crop + (3,)
  for n, (top, left) in enumerate(windows):
    assert torch.equal(got[n], full[n, top:top + crop[0], left:left + crop[1]]), n
  # the fp32 store of a window, and one window for a group of images
  tab_w, tab_h = G._pil_tables(src[0], src[1], dst[0], dst[1], images.device)
  one = win[2:].to(DEV)
  u8, f32 = G._HF.images_u8_resize_pil(images, dst, tab_w, tab_h, lut=G._norm_lut(images.device), windows=one, per_window=3, crop=crop, want_f32=True)
  top, left = windows[2]
  for n in range(N):
    want = full[n, top:top + crop[0], left:left + crop[1]]
    assert torch.equal(u8[n], want) and torch.equal(f32[n].cpu(), TRANSFORM(want.cpu().numpy())), n
  # the disparity takes the same windows
  d = torch.from_numpy(_disp(N, src[0], src[1], 3)).to(DEV)
  rows, cols = G._axis_table('nearest', src[0], dst[0], d.device), G._axis_table('nearest', src[1], dst[1], d.device)
  dfull = G._HF.disp_resize_nearest(d, dst, rows, cols, dst[1] / src[1])
  dwin = G._HF.disp_resize_nearest(d, dst, rows, cols, dst[1] / src[1], windows=win.to(DEV), crop=crop)
  for n, (top, left) in enumerate(windows):
    assert torch.equal(dwin[n].view(torch.int32), dfull[n, top:top + crop[0], left:left + crop[1]].view(torch.int32)), n
  with pytest.raises(ValueError, match='outside'):
    G.resize_u8_gpu(images, dst, windows=torch.tensor([[0, 0], [0, 0], [dst[0] - crop[0] + 1, 0]]), crop=crop)


@pytest.mark.parametrize('src,dst', [((64, 32), (32, 16)), ((64, 32), (128, 64)), ((37, 23), (50, 9)), ((64, 32), (24, 12))])
def test_disparity_is_the_host_loaders(src, dst):
  """Bit-equal to resize_nearest(d, w, h) * (w / Ws) as numpy computes it in float32, NaNs and zeros where it has them."""
  d = _disp(N, src[0], src[1], 11)
  want = np.stack([L.resize_nearest(m, dst[1], dst[0]) * (dst[1] / src[1]) for m in d])
  assert want.dtype == np.float32 and np.isnan(want).any() and (want == 0).any()
  dev = torch.from_numpy(d).to(DEV)
  rows, cols = G._axis_table('nearest', src[0], dst[0], dev.device), G._axis_table('nearest', src[1], dst[1], dev.device)
  got = G._HF.disp_resize_nearest(dev, dst, rows, cols, dst[1] / src[1]).cpu().numpy()
  assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
  ok = ~np.isnan(want)
  assert np.array_equal(got[ok].view(np.int32), want[ok].view(np.int32))


def _write_pairs(d, n, h, w):
  rng = np.random.RandomState(31)
  lists = ([], [], [])
  for i in range(n):
    for k, side in enumerate('ab'):
      lists[k].append(os.path.join(str(d), 'p%d_%s.png' % (i, side)))
      Image.fromarray(R.image('random' if i else 'binary', h, w, seed=10 * i + k)).save(lists[k][-1])
    disp = (rng.rand(h, w) * 30).astype(np.float32)
    disp[rng.rand(h, w) < 0.1] = np.nan
    lists[2].append(os.path.join(str(d), 'p%d_disp.npz' % i))
    np.savez(lists[2][-1], disp)
  return lists


def _same(got, want):
  """Bit for bit where the host has numbers, NaN where it has NaN."""
  got, want = got.cpu(), want.cpu()
  return tuple(got.shape) == tuple(want.shape) and torch.equal(got.isnan(), want.isnan()) and torch.equal(got.nan_to_num(-1.0), want.nan_to_num(-1.0))


def test_pairs_are_the_host_loaders_items(tmp_path):
  lists = _write_pairs(tmp_path, 2, 64, 32)
  host = L.Deep360DatasetDisparity(*lists, shape=(32, 16))
  dev = L.Deep360DatasetDisparity(*lists, shape=(32, 16), device_ingest=True)
  batch = next(iter(torch.utils.data.DataLoader(dev, batch_size=2)))
  want = next(iter(torch.utils.data.DataLoader(host, batch_size=2)))
  pairs, disp = batch['pair_u8'].to(DEV), batch['disp'].to(DEV)
  got = G.pairs_u8_gpu(pairs, disp, shape=(32, 16))
  assert sorted(got) == ['dispMap', 'leftImg', 'rightImg'] and batch['dispNames'] == want['dispNames']
  for k in ('leftImg', 'rightImg'):
    assert got[k].is_contiguous() and tuple(got[k].shape) == (2, 3, 32, 16) and torch.equal(got[k].cpu(), want[k]), k
  assert tuple(got['dispMap'].shape) == (2, 1, 32, 16) and bool(want['dispMap'].isnan().any()) and _same(got['dispMap'], want['dispMap'])
  assert sorted(G.pairs_u8_gpu(pairs, shape=(32, 16))) == ['leftImg', 'rightImg']
  # the stored size: no resize, as the loader's _fit; equal widths with another height are refused as there is nothing to mirror
  same = G.pairs_u8_gpu(pairs, disp, shape=(64, 32))
  full = next(iter(torch.utils.data.DataLoader(L.Deep360DatasetDisparity(*lists, shape=(64, 32)), batch_size=2)))
  assert all(_same(same[k], full[k]) for k in ('leftImg', 'rightImg', 'dispMap'))
  with pytest.raises(ValueError, match='height'):
    G.pairs_u8_gpu(pairs, disp, shape=(48, 32))
  # the training crop: one window per sample, shared by left, right and disparity
  win = G.draw_crop_windows(2, (32, 16), (12, 8), generator=torch.Generator().manual_seed(1))
  crop = G.pairs_u8_gpu(pairs, disp, shape=(32, 16), crop=(12, 8), windows=win)
  for n, (top, left) in enumerate(win.tolist()):
    for k in ('leftImg', 'rightImg', 'dispMap'):
      assert _same(crop[k][n], want[k][n][:, top:top + 12, left:left + 8]), (n, k)
  with pytest.raises(ValueError, match='together'):
    G.pairs_u8_gpu(pairs, disp, shape=(32, 16), crop=(12, 8))
  # with augment= the resize writes bytes and the augmentation's kernels follow: the same done by hand
  p = G.draw_colour_params(4, DEV, generator=torch.Generator().manual_seed(2))
  aug = G.pairs_u8_gpu(pairs, disp, shape=(32, 16), augment=p)
  hand = G.augment_u8_gpu(G.resize_u8_gpu(pairs, (32, 16)).view(4, 32, 16, 3), p).view(2, 2, 3, 32, 16)
  assert torch.equal(aug['leftImg'], hand[:, 0]) and torch.equal(aug['rightImg'], hand[:, 1]) and not torch.equal(aug['leftImg'], got['leftImg'])
  assert _same(aug['dispMap'], want['dispMap'])
  caug = G.pairs_u8_gpu(pairs, disp, shape=(32, 16), crop=(12, 8), windows=win, augment=p)
  hand = G.augment_u8_gpu(G.resize_u8_gpu(pairs, (32, 16), windows=win.repeat_interleave(2, 0), crop=(12, 8)).view(4, 12, 8, 3), p).view(2, 2, 3, 12, 8)
  assert torch.equal(caug['leftImg'], hand[:, 0]) and torch.equal(caug['rightImg'], hand[:, 1]) and _same(caug['dispMap'], crop['dispMap'])


def test_pairs_replay_from_a_captured_graph():
  """The tables are uploaded by the first eager call; after it the call captures, and new bytes and new windows in the same buffers
  give the eager result."""
  rng = np.random.RandomState(17)
  mk = lambda: (torch.from_numpy(rng.randint(0, 256, (2, 2, 64, 32, 3)).astype(np.uint8)).to(DEV), torch.from_numpy(_disp(2, 64, 32, rng.randint(99))).to(DEV),
                G.draw_crop_windows(2, (24, 12), (10, 6), generator=torch.Generator().manual_seed(int(rng.randint(99)))).to(DEV))
  first, second = mk(), mk()
  static = [t.clone() for t in first]
  call = lambda b: G.pairs_u8_gpu(b[0], b[1], shape=(24, 12), crop=(10, 6), windows=b[2])
  eager = call(static)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    out = call(static)
  for batch in (first, second):
    for s, t in zip(static, batch):
      s.copy_(t)
    want = call(batch)
    graph.replay()
    torch.cuda.synchronize()
    for k in want:
      assert _same(out[k], want[k]), k
  assert sorted(eager) == sorted(out) and not _same(call(first)['leftImg'], call(second)['leftImg'])
  del graph
  for c in (G._resize_cache, G._lut_cache, G._dst_cache):
    c.release_graph_pins()
