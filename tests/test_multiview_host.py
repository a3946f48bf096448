"""ModeMultiView and the multi-view hand-off, CPU tier: module contract, checkpoint loading, frame selection, frame lists, the 8-bit
confidence rule and the host-side argument checks of the C-ABI entries (no launch)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import deep360_tree
import mode_hip
import models
from dataloader import list_file
from models import mode_multiview
from utils import geometry as HG

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _manifest(name):
  with open(os.path.join(GOLDEN, name)) as f:
    return [k for k, _ in json.load(f)]


def _tiny(fusion='ModeFusion'):
  return models.ModeMultiView(16, 10., 64, 32, fusion=fusion, channels=(8, 16, 32, 64))


def test_state_dict_keys_are_the_two_manifests():
  net = _tiny()
  want = ['disparity.' + k for k in _manifest('manifest_mode_disparity.json')] + ['fusion.' + k for k in _manifest('manifest_mode_fusion.json')]
  assert len(want) == 483 + 251
  assert list(net.state_dict().keys()) == want
  base = _tiny('Baseline')
  assert all(k.startswith('disparity.') or k.startswith('fusion.feature_extraction.') for k in base.state_dict())


@pytest.mark.parametrize('prefix', ['', 'module.'])
def test_load_checkpoints_round_trip(tmp_path, prefix):
  src, dst = _tiny(), _tiny()
  g = torch.Generator().manual_seed(3)
  with torch.no_grad():
    for p in src.parameters():
      p.copy_(torch.randn(p.shape, generator=g))
  disp_ck, fus_ck = tmp_path / 'disp.tar', tmp_path / 'fusion.tar'
  # the format of the reference's training scripts: {'epoch', 'state_dict', ...}, DataParallel's 'module.' on every key
  torch.save({'epoch': 7, 'state_dict': {prefix + k: v for k, v in src.disparity.state_dict().items()}, 'train_loss': 0.5}, disp_ck)
  torch.save({'epoch': 3, 'state_dict': {prefix + k: v for k, v in src.fusion.state_dict().items()}}, fus_ck)
  dst.load_checkpoints(disp=str(disp_ck), fusion=str(fus_ck))
  for k, v in src.state_dict().items():
    assert torch.equal(dst.state_dict()[k], v), k
  # dicts are taken too, and None leaves a child alone
  third = _tiny()
  third.load_checkpoints(fusion={'state_dict': src.fusion.state_dict()})
  assert all(torch.equal(third.fusion.state_dict()[k], v) for k, v in src.fusion.state_dict().items())
  assert not torch.equal(third.disparity.dres0[0][0].weight, src.disparity.dres0[0][0].weight)


def test_frame_selection():
  """Pair p of frame f is (frames[f, 2p], frames[f, 2p + 1]) at batch index 6f + p; the fusion RGB is panoramas 0, 1, 10, 11."""
  F, H, W = 3, 2, 4
  ids = torch.arange(F * 12, dtype=torch.float32).view(F, 12, 1, 1, 1).expand(F, 12, 3, H, W).contiguous()
  left, right, rgb = mode_multiview.split_frames(ids)
  assert left.shape == right.shape == (6 * F, 3, H, W) and rgb.shape == (F, 12, H, W)
  for f in range(F):
    for p in range(6):
      assert bool((left[6 * f + p] == 12 * f + 2 * p).all()) and bool((right[6 * f + p] == 12 * f + 2 * p + 1).all())
    for k, pano in enumerate((0, 1, 10, 11)):
      assert bool((rgb[f, 3 * k:3 * k + 3] == 12 * f + pano).all())
  assert mode_multiview.FUSION_RGB == list_file._FUSION_RGB  # the positions the fusion lists take the RGB from
  with pytest.raises(ValueError):
    mode_multiview.split_frames(ids[:, :6])


@pytest.mark.parametrize('soiled', [False, True])
def test_list_deep360_frames(tmp_path, soiled):
  dataset, _, _ = deep360_tree.build(str(tmp_path), soiled=True)
  for subset, names in deep360_tree.FRAMES.items():
    frames = list_file.list_deep360_frames(dataset, subset, soiled=soiled)
    assert len(frames) == 6 * len(names)
    want_frames = []
    for ep in range(1, 7):
      for fr in sorted(names):
        name = 'ep%d_%s' % (ep, fr)
        sfx = '_soiled' if soiled else ''
        rgbs = [os.path.join(dataset, 'ep%d_500frames' % ep, subset, 'rgb' + sfx, '%s_%s_rgb%s%s.png' % (name, p, cam, sfx))
                for p in deep360_tree.PAIRS for cam in p]
        gt = os.path.join(dataset, 'ep%d_500frames' % ep, subset, 'depth', name + '_depth.npz')
        want_frames.append((rgbs, gt))
    assert frames == want_frames
  import dataloader
  assert dataloader.list_deep360_frames is list_file.list_deep360_frames


def test_conf_png_rule():
  """q(c) = float32(float64(clip(rint(c * 255), 0, 255)) / 255): half to even on exact .5 products, saturation at both ends."""
  c = np.array([0.5 / 255, 1.5 / 255, 2.5 / 255, 0.0, 1.0, -0.3, 1.7, 0.25, 0.75, 0.999], dtype=np.float32)
  prod = c * np.float32(255)
  got = HG.conf_png_np(c)
  want = (np.clip(np.rint(prod), 0, 255) / 255.0).astype(np.float32)
  assert np.array_equal(got, want)
  # c * 255 lands exactly on k + .5 for these: rint goes to the even neighbour
  halves = np.array([k + 0.5 for k in range(0, 255)], dtype=np.float32) / np.float32(255)
  exact = (halves * np.float32(255)) == np.float32(np.arange(255) + 0.5)
  q = HG.conf_png_np(halves)[exact]
  k = np.arange(255)[exact]
  assert exact.sum() > 100 and np.array_equal(np.rint(q.astype(np.float64) * 255), np.where(k % 2 == 0, k, k + 1).astype(np.float64))
  assert HG.conf_png_np(np.float32(0.5)) == np.float32(128 / 255.0)  # 127.5 -> 128


def test_handoff_entries_validate_on_the_host():
  lib = mode_hip.lib()
  assert lib.mode_multiview_handoff_workspace_bytes(2, 64, 32) == 3 * 2 * 64 * 32 * 8
  assert lib.mode_multiview_handoff_workspace_bytes(0, 64, 32) == 0
  assert lib.mode_multiview_handoff_workspace_bytes(1, -1, 32) == 0
  null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
  b6 = (ctypes.c_float * 6)(*[1.0] * 6)
  xf = (ctypes.c_double * 36)()

  def call(F=1, H=64, W=32, disp=one, conf=one, base=ctypes.cast(b6, ctypes.c_void_p), grids=one, trig=one,
           x=ctypes.cast(xf, ctypes.c_void_p), flags=0, out=one, ws=one):
    return lib.mode_multiview_handoff(disp, conf, F, H, W, base, grids, trig, x, flags, out, ws, null)

  assert call(F=-1) == -1 and b'bad size' in lib.mode_last_error()
  assert call(H=0) == -1 and call(W=-4) == -1
  assert call(F=1 << 10, H=1024, W=1024) == -1 and b'bad size' in lib.mode_last_error()  # 3 F H W >= 2^31
  assert call(flags=4) == -1 and b'flags' in lib.mode_last_error()
  for kw in ('disp', 'conf', 'base', 'grids', 'trig', 'x', 'out'):
    assert call(**{kw: null}) == -1 and b'null pointer' in lib.mode_last_error(), kw
  assert call(grids=ctypes.c_void_p(20)) == -1
  assert call(ws=null) == -3 and b'workspace' in lib.mode_last_error()
  assert call(ws=ctypes.c_void_p(20)) == -3 and b'workspace' in lib.mode_last_error()
  assert call(F=0, disp=null, conf=null, out=null, ws=null) == 0  # nothing to do


def test_cpu_tensors_are_refused():
  with pytest.raises(NotImplementedError):
    HG.disp2depth_frames_gpu(torch.zeros(1, 6, 64, 32), torch.zeros(1, 6, 64, 32))
  net = _tiny().eval()
  with pytest.raises(NotImplementedError):
    net(torch.zeros(1, 12, 3, 64, 32))
  with pytest.raises(RuntimeError, match='inference only'):
    net.train()(torch.zeros(1, 12, 3, 64, 32))


def test_sizes_and_databases_are_refused():
  with pytest.raises(ValueError):
    models.ModeMultiView(16, 10., 72, 40)
  with pytest.raises(ValueError):
    models.ModeMultiView(16, 10., 64, 32, dbname='3D60')
  with pytest.raises(ValueError):
    HG._as_frames(torch.zeros(7, 1, 4, 4), 'disp')
  assert HG._as_frames(torch.zeros(12, 4, 4), 'disp').shape == (2, 6, 4, 4)
  assert HG._as_frames(torch.zeros(12, 1, 4, 4), 'disp').shape == (2, 6, 4, 4)
