"""8-bit ingest, GPU tier: mode_frames_u8_ingest, mode_rgb_half_pil and mode_decimate2 against the host code they replace, and
ModeMultiView on uint8 frames with and without the half-resolution fusion path.

Every comparison is torch.equal: each piece is integer arithmetic, a table lookup, a copy, or a kernel that both sides of the comparison
call.  The references (Pillow, the host transform, split_frames) are in tests/ingest_ref.py."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import ingest_ref as R
import recipe

import models
from dataloader import gpu_ingest
from mode_hip import functional as HF
from utils import geometry as HG
from utils import panorama

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('size', [(32, 16), (48, 32)])  # (H, W); 48 x 32 = 384 quads per panorama: one and a half blocks
def test_frames_u8_ingest_is_the_host_transform_and_split(size):
  H, W = size
  frames = R.frames_u8(2, H, W, 5 + H)  # F = 2: the frame stride matters; every byte value in every channel
  wl, wr, wrgb = R.host_split(frames)
  dev = torch.from_numpy(frames).to(DEV)
  left, right, rgb = gpu_ingest.frames_u8_gpu(dev)
  assert left.shape == right.shape == (12, 3, H, W) and rgb.shape == (2, 12, H, W)
  assert torch.equal(left.cpu(), wl) and torch.equal(right.cpu(), wr) and torch.equal(rgb.cpu(), wrgb)
  l2, r2, none = gpu_ingest.frames_u8_gpu(dev, want_rgb=False)
  assert none is None and torch.equal(l2, left) and torch.equal(r2, right)
  assert all(t.shape[0] == 0 for t in gpu_ingest.frames_u8_gpu(dev[:0]))  # F = 0: nothing launched
  with pytest.raises(TypeError):
    gpu_ingest.frames_u8_gpu(dev.float())
  with pytest.raises(TypeError):
    gpu_ingest.frames_u8_gpu(dev.transpose(2, 3))
  with pytest.raises(ValueError):
    gpu_ingest.frames_u8_gpu(dev[:, :6].contiguous())


@pytest.mark.parametrize('kind', ['random', 'binary'])
@pytest.mark.parametrize('size', [(32, 16), (96, 80)])  # (H, W): 8 output columns hold every edge row and the interior row; tile remainders
def test_rgb_half_is_pillow_then_the_host_transform(size, kind):
  H, W = size
  frames = R.frames_u8(2, H, W, 9 + H, kind)
  want_u8, want = R.host_rgb_half(frames)
  dev = torch.from_numpy(frames).to(DEV)
  got, got_u8 = gpu_ingest.rgb_half_gpu(dev, return_u8=True)
  assert got_u8.shape == (2, 4, H // 2, W // 2, 3) and got.shape == (2, 12, H // 2, W // 2)
  for f in range(2):
    for k in range(4):
      bad = int((got_u8[f, k].cpu() != want_u8[f, k]).sum())
      assert bad == 0, 'frame %d panorama %d: %d bytes differ from Pillow' % (f, models.mode_multiview.FUSION_RGB[k], bad)
  assert torch.equal(got.cpu(), want)
  assert torch.equal(gpu_ingest.rgb_half_gpu(dev), got)  # without the 8-bit output
  assert gpu_ingest.rgb_half_gpu(dev[:0]).shape == (0, 12, H // 2, W // 2)
  with pytest.raises(TypeError):
    gpu_ingest.rgb_half_gpu(dev.float())


def test_full_size_frame():
  """One 1024 x 512 frame (the size the module is used at): 256 tiles per panorama, byte offsets up to 18.9 MB."""
  H, W = 1024, 512
  rng = np.random.RandomState(77)
  frames = rng.randint(0, 256, (1, 12, H, W, 3)).astype(np.uint8)
  frames[0, 11] = R.images(H, W, 78)['binary']  # the last panorama: the clip, and the last rows of the buffer
  dev = torch.from_numpy(frames).to(DEV)
  want_u8, want = R.host_rgb_half(frames)
  got, got_u8 = gpu_ingest.rgb_half_gpu(dev, return_u8=True)
  assert torch.equal(got_u8.cpu(), want_u8) and torch.equal(got.cpu(), want)
  left, right, rgb = gpu_ingest.frames_u8_gpu(dev)
  wl, wr, wrgb = R.host_split(frames)
  assert torch.equal(left.cpu(), wl) and torch.equal(right.cpu(), wr) and torch.equal(rgb.cpu(), wrgb)
  full = torch.randn(1, 12, H, W, generator=torch.Generator().manual_seed(79))
  assert torch.equal(HF.decimate2(full.to(DEV)).cpu(), full[..., ::2, ::2])


@pytest.mark.parametrize('shape', [(3, 6, 10), (24, 32, 16), (2, 5, 7)])  # scalar path, 16-byte path, odd sizes (ceil, as slicing)
def test_decimate2_is_slicing(shape):
  x = torch.randn(shape, generator=torch.Generator().manual_seed(sum(shape)))
  y = HF.decimate2(x.to(DEV))
  assert torch.equal(y.cpu(), x[..., ::2, ::2]) and y.is_contiguous()
  x4 = x.view((1,) + shape)
  assert torch.equal(HF.decimate2(x4.to(DEV)).cpu(), x4[..., ::2, ::2])
  assert HF.decimate2(x4[:0].to(DEV)).shape == (0, shape[0], (shape[1] + 1) // 2, (shape[2] + 1) // 2)


# ------------------------------------------------------------------------------------------------------------ ModeMultiView
def _disparity_state():
  z = np.load(os.path.join(recipe.HERE, 'model_wc_tiny.npz'))
  sd = recipe.fixture_state(z)
  sd.update({k[3:]: torch.from_numpy(z[k]).clone() for k in z.files if k.startswith('bn/')})
  return [int(v) for v in z['cfg'][:3]], sd


def _tiny_net(fusion, resize):
  """The tiny configuration of tests/test_gpu_multiview.py: model_wc_tiny's disparity state and fusion_tiny's recipe state."""
  (maxdisp, H, W), sd = _disparity_state()
  zf = np.load(os.path.join(recipe.HERE, 'fusion_tiny.npz'))
  cfg = zf['cfg']
  maxdepth, seed, channels = float(cfg[0]), int(cfg[4]), tuple(int(c) for c in cfg[5:])
  net = models.ModeMultiView(maxdisp, maxdepth, H, W, fusion=fusion, channels=channels, resize=resize)
  net.disparity.load_state_dict(sd)
  if fusion == 'ModeFusion':
    net.fusion.load_state_dict(recipe.recipe_state([(k, tuple(s)) for k, s in json.loads(str(zf['manifest']))], seed))
  return net.to(DEV).eval(), H, W


@functools.lru_cache(None)
def _frames(H, W):
  """Two uint8 frames and their host-normalised float form (computed once, never modified)."""
  frames = R.frames_u8(2, H, W, 61)
  return frames, R.host_frames(frames)


@pytest.mark.parametrize('fusion', ['ModeFusion', 'Baseline'])
def test_uint8_forward_is_the_float_forward_on_the_normalised_frames(fusion):
  net, H, W = _tiny_net(fusion, False)
  frames, normalised = _frames(H, W)
  want, wst = net(normalised.to(DEV), return_stages=True)
  got, gst = net(torch.from_numpy(frames).to(DEV), return_stages=True)
  assert got.shape == (2, 1, H, W)
  for k in ('disp', 'conf', 'fusion_input'):
    assert torch.equal(gst[k], wst[k]), k
  assert torch.equal(got, want)


@pytest.mark.parametrize('fusion', ['ModeFusion', 'Baseline'])
def test_resize_forward_is_the_composition_done_by_hand(fusion):
  net, H, W = _tiny_net(fusion, True)
  frames, normalised = _frames(H, W)
  dev = torch.from_numpy(frames).to(DEV)
  got, st = net(dev, return_stages=True)
  assert got.shape == (2, 1, H, W)
  left, right, _ = models.mode_multiview.split_frames(normalised.to(DEV))
  with torch.no_grad():
    disp, conf = net.disparity(left, right)
    full = HG.disp2depth_frames_gpu(disp, conf, conf_png=True, depth_only=fusion == 'Baseline')
    half = full[..., ::2, ::2].contiguous()
    assert torch.equal(st['disp'], disp) and torch.equal(st['conf'], conf) and torch.equal(st['fusion_input'], half)
    if fusion == 'ModeFusion':
      rgb = R.host_rgb_half(frames)[1].to(DEV)  # Pillow-halved panoramas, normalised on the host
      assert torch.equal(st['rgb'], rgb)
      depth_half = net.fusion.feature_extraction(half, rgb)
    else:
      assert st['rgb'] is None
      depth_half = net.fusion.feature_extraction(half)
    assert depth_half.shape == (2, 1, H // 2, W // 2)
    want = panorama.bicubic_up2(depth_half)
  assert torch.equal(got, want)
  assert torch.equal(net(dev), got)
  # evaluate returns the rows of erp_depth_metrics on that result
  gt = (torch.rand(2, H, W, generator=torch.Generator().manual_seed(3)) * 1.2 * net.maxdepth).to(DEV)
  erp, rows = net.evaluate(dev, gt)
  want_rows, want_erp, _ = panorama.erp_depth_metrics(got, gt, net.maxdepth, return_erp=True)
  assert rows.shape == (2, 8) and rows.tobytes() == want_rows.tobytes() and torch.equal(erp, want_erp)
  with pytest.raises(ValueError, match='8-bit images'):
    net(normalised.to(DEV))


def test_ingest_replays_from_a_captured_graph():
  """Tables are uploaded on the first eager call and cached: the three kernels, and the resize=True forward around them, capture into a
  hipGraph and replay on new frames with the eager results."""
  from mode_hip.graph_step import GraphedStep
  H, W = 96, 80
  first, second = (torch.from_numpy(R.frames_u8(2, H, W, s)).to(DEV) for s in (91, 92))
  maps = torch.randn(2, 12, H, W, generator=torch.Generator().manual_seed(93)).to(DEV)

  def pieces(frames):
    return gpu_ingest.frames_u8_gpu(frames) + (gpu_ingest.rgb_half_gpu(frames), HF.decimate2(maps))

  static = first.clone()
  step = GraphedStep(lambda: pieces(static), static_inputs=(static,))
  for frames in (first, second, first):
    step.load(frames)
    out = step.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, pieces(frames)))
  net, H, W = _tiny_net('Baseline', True)
  a, b = (torch.from_numpy(R.frames_u8(1, H, W, s)).to(DEV) for s in (94, 95))
  static = a.clone()
  step = GraphedStep(lambda: net(static), static_inputs=(static,))
  for frames in (a, b):
    step.load(frames)
    out = step.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, net(frames))
