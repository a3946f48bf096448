"""ModeMultiView and the multi-view hand-off (mode_multiview_handoff), GPU tier.

The hand-off is checked bit for bit against the single-pair path it replaces (six disp2depth_gpu calls + the interleave), against
the reference function's own outputs, for frame independence and for repeatability (second call, side stream, graph replay).  The
composed module is checked stage by stage on its OWN intermediates: z-buffer winners and rounded target pixels are discontinuous in
the depth, so an end-to-end comparison with an all-oracle chain would depend on the last bit of the disparity."""
import json
import os

import numpy as np
import pytest
import torch

import recipe
from oracle import fusion_ref, mode_ref

import models
from utils import geometry as HG

DEV = 'cuda:0'
PAIRS = ('12', '13', '14', '23', '24', '34')


def _inputs(F, H, W, seed):
  """Disparities with zeros, near-zero values (depth far beyond the 1000 m clip) and values up to a quarter of the width."""
  g = torch.Generator().manual_seed(seed)
  disp = torch.rand(F, 6, H, W, generator=g) * (W / 4)
  u = torch.rand(F, 6, H, W, generator=g)
  disp[u < 0.1] = 0
  tiny = (u >= 0.1) & (u < 0.2)
  disp[tiny] = torch.rand(int(tiny.sum()), generator=g) * 1e-2
  conf = torch.rand(F, 6, H, W, generator=g)
  return disp.to(DEV), conf.to(DEV)


def _six_calls(disp, conf, dbname, conf_png=False):
  """What a user writes by hand today: six disp2depth_gpu calls per frame and ModeFusion's interleave."""
  frames = []
  for f in range(disp.shape[0]):
    chans = []
    for p, pair in enumerate(PAIRS):
      d, c = HG.disp2depth_gpu(disp[f, p].contiguous(), conf[f, p].contiguous(), pair, dbname)
      if conf_png:
        c = torch.from_numpy(HG.conf_png_np(c.cpu().numpy())).to(DEV)
      chans += [d, c]
    frames.append(torch.stack(chans))
  return torch.stack(frames)


@pytest.mark.gpu
@pytest.mark.parametrize('dbname', ['Deep360', 'other'])
@pytest.mark.parametrize('size', [(64, 32), (1024, 512)])
@pytest.mark.parametrize('F', [1, 3])
def test_handoff_is_the_six_pair_path_bit_for_bit(F, size, dbname):
  H, W = size
  disp, conf = _inputs(F, H, W, 5 + F + H)
  want = _six_calls(disp, conf, dbname)
  got = HG.disp2depth_frames_gpu(disp, conf, dbname)
  assert got.shape == (F, 12, H, W)
  for p, pair in enumerate(PAIRS):
    assert torch.equal(got[:, 2 * p], want[:, 2 * p]), 'depth of pair %s' % pair
    assert torch.equal(got[:, 2 * p + 1], want[:, 2 * p + 1]), 'confidence of pair %s' % pair
  depth = want[:, 0::2]
  assert bool((depth == 1000).any()) and bool(((depth > 0) & (depth < 1000)).any())  # the clip and the ordinary range both taken
  # the other layouts of the input are views of the same maps
  assert torch.equal(HG.disp2depth_frames_gpu(disp.view(6 * F, 1, H, W), conf.view(6 * F, H, W), dbname), got)
  png = HG.disp2depth_frames_gpu(disp, conf, dbname, conf_png=True)
  assert torch.equal(png, _six_calls(disp, conf, dbname, conf_png=True))
  assert torch.equal(png[:, 0::2], got[:, 0::2])
  assert torch.equal(HG.disp2depth_frames_gpu(disp, conf, dbname, depth_only=True), got[:, 0::2])
  assert HG.disp2depth_frames_gpu(disp[:0], conf[:0], dbname).shape == (0, 12, H, W)


@pytest.mark.gpu
@pytest.mark.parametrize('dbname', ['Deep360', 'other'])
def test_handoff_against_the_reference_function(golden, dbname):
  """tests/golden/disp2depth.npz (the reference's own disp2depth) in all six slots, with the per-pair tolerances of
  tests/test_geometry.py."""
  z = golden('disp2depth.npz')
  d0, c0 = torch.from_numpy(z['disp']).to(DEV), torch.from_numpy(z['conf']).to(DEV)
  out = HG.disp2depth_frames_gpu(d0.expand(1, 6, *d0.shape).contiguous(), c0.expand(1, 6, *c0.shape).contiguous(), dbname)
  out = out[0].cpu().numpy()
  for p, pair in enumerate(PAIRS):
    d, c = out[2 * p], out[2 * p + 1]
    rd, rc = z['%s/%s/depth' % (dbname, pair)], z['%s/%s/conf' % (dbname, pair)]
    if pair == '12':
      far = rd >= 999
      assert (np.abs(d - rd)[~far] <= 1e-4 * np.maximum(np.abs(rd[~far]), 1e-3)).all()
      assert (np.abs(d[far] - rd[far]) < 1).all() and np.array_equal(c, z['conf'])
    elif pair in ('13', '14'):
      assert np.median(np.abs(d - rd)) < 1e-4 and np.abs(c - rc).max() < 1e-5
    else:
      assert abs((d > 0).mean() - (rd > 0).mean()) < 0.05
      assert np.allclose(np.sort(d[d > 0])[::37][:20], np.sort(rd[rd > 0])[::37][:20], rtol=0.05)


@pytest.mark.gpu
def test_frames_are_independent():
  """Frame 1 a copy of frame 0: both halves identical, and frame 0 of the F = 2 call is the F = 1 call (key-plane offsets)."""
  disp, conf = _inputs(1, 128, 64, 21)
  d2, c2 = torch.cat((disp, disp)), torch.cat((conf, conf))
  for kw in ({}, {'conf_png': True}, {'depth_only': True}):
    one = HG.disp2depth_frames_gpu(disp, conf, **kw)
    two = HG.disp2depth_frames_gpu(d2, c2, **kw)
    assert torch.equal(two[0], two[1]) and torch.equal(two[:1], one)


@pytest.mark.gpu
def test_handoff_repeats_bit_for_bit():
  from mode_hip.graph_step import GraphedStep
  disp, conf = _inputs(2, 256, 128, 33)
  first = HG.disp2depth_frames_gpu(disp, conf, conf_png=True)
  assert torch.equal(HG.disp2depth_frames_gpu(disp, conf, conf_png=True), first)
  side = torch.cuda.Stream(DEV)
  side.wait_stream(torch.cuda.current_stream(DEV))
  with torch.cuda.stream(side):
    on_side = HG.disp2depth_frames_gpu(disp, conf, conf_png=True)
  torch.cuda.current_stream(DEV).wait_stream(side)
  torch.cuda.synchronize()
  assert torch.equal(on_side, first)
  sd, sc = disp.clone(), conf.clone()
  step = GraphedStep(lambda: HG.disp2depth_frames_gpu(sd, sc, conf_png=True), static_inputs=(sd, sc))
  for _ in range(2):  # a replay refills the key planes (a kernel node, not a memset)
    out = step.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, first)
  d2, c2 = _inputs(2, 256, 128, 34)
  step.load(d2, c2)
  out = step.replay()
  torch.cuda.synchronize()
  assert torch.equal(out, HG.disp2depth_frames_gpu(d2, c2, conf_png=True))


def _disparity_state(name):
  """(maxdisp, H, W, state) of a well-conditioned whole-model fixture, its running statistics (the batch statistics of its own
  pair) included: an eval forward on them stays in the range the parity tests measure."""
  z = np.load(os.path.join(recipe.HERE, name))
  sd = recipe.fixture_state(z)
  for k in z.files:
    if k.startswith('bn/'):
      sd[k[3:]] = torch.from_numpy(z[k]).clone()
  maxdisp, H, W = [int(v) for v in z['cfg'][:3]]
  return maxdisp, H, W, sd


def _tiny_net(fusion='ModeFusion'):
  """model_wc_tiny's disparity state and fusion_tiny's recipe state."""
  maxdisp, H, W, sd = _disparity_state('model_wc_tiny.npz')
  zf = np.load(os.path.join(recipe.HERE, 'fusion_tiny.npz'))
  cfg = zf['cfg']
  maxdepth, seed, channels = float(cfg[0]), int(cfg[4]), tuple(int(c) for c in cfg[5:])
  manifest = [(k, tuple(s)) for k, s in json.loads(str(zf['manifest']))]
  net = models.ModeMultiView(maxdisp, maxdepth, H, W, fusion=fusion, channels=channels)
  net.disparity.load_state_dict(sd)
  if fusion == 'ModeFusion':
    net.fusion.load_state_dict(recipe.recipe_state(manifest, seed))
  return net.to(DEV).eval(), sd, maxdisp, maxdepth, H, W


def _frames(F, H, W, seed):
  left, right = recipe.recipe_images(6 * F, H, W, seed)
  frames = torch.stack((left.view(F, 6, 3, H, W), right.view(F, 6, 3, H, W)), dim=2).reshape(F, 12, 3, H, W)
  return frames, left, right


@pytest.mark.gpu
def test_end_to_end_stage_by_stage():
  net, sd, maxdisp, maxdepth, H, W = _tiny_net()
  F = 2
  frames, left, right = _frames(F, H, W, 41)
  depth, st = net(frames.to(DEV), return_stages=True)
  assert depth.shape == (F, 1, H, W)
  disp, conf, fi = st['disp'], st['conf'], st['fusion_input']
  assert disp.shape == conf.shape == (6 * F, 1, H, W) and fi.shape == (F, 12, H, W)
  # a) stage 1 against the float64 oracle, per pair
  P64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
  pos = mode_ref.sphere_position(H // 4, W // 4, 'Cassini')
  rdisp, rconf = mode_ref.mode_disparity(P64, left.double(), right.double(), maxdisp, pos, False, out_conf=True)
  derr = (disp.cpu().double() - rdisp).abs()
  print('stage 1: max |disp - oracle64| per pair %s' % [float(derr[i].max()) for i in range(6 * F)])
  assert float(derr.max()) <= 1e-3
  stable = (rdisp - rdisp.round()).abs().sub(0.5).abs() > 1e-3  # round(d) may flip at half-integers
  assert float((conf.cpu().double() - rconf).abs()[stable].max()) <= 1e-3
  # b) the hand-off is disp2depth_frames_gpu on the module's own stage-1 output
  assert torch.equal(fi, HG.disp2depth_frames_gpu(disp, conf, conf_png=True))
  # c) stage 2 against the float64 oracle on the module's own hand-off (the bound of tests/test_fusion.py: within 3x / 2x of what
  #    the fp32 evaluation of the same network achieves)
  rgb = frames[:, [0, 1, 10, 11]].reshape(F, 12, H, W)
  fin = fi.cpu()
  depthes = [fin[:, 2 * p:2 * p + 1] for p in range(6)]
  confs = [fin[:, 2 * p + 1:2 * p + 2] for p in range(6)]
  rgbs = [rgb[:, 3 * k:3 * k + 3] for k in range(4)]
  Pf = {k: v.cpu() for k, v in net.fusion.state_dict().items()}  # feature_extraction.*, the oracle's keys
  Pf64 = {k: (v.double() if v.is_floating_point() else v) for k, v in Pf.items()}
  truth = fusion_ref.mode_fusion(Pf64, [t.double() for t in depthes], [t.double() for t in confs], [t.double() for t in rgbs], maxdepth,
                                 False).numpy()
  ref32 = fusion_ref.mode_fusion(Pf, depthes, confs, rgbs, maxdepth, False).numpy().astype(np.float64)
  err, ref_err = np.abs(depth.cpu().numpy().astype(np.float64) - truth), np.abs(ref32 - truth)
  print('stage 2: |gpu - oracle64| max %.2e mean %.2e; fp32 oracle max %.2e mean %.2e' % (err.max(), err.mean(), ref_err.max(), ref_err.mean()))
  assert err.max() <= max(1e-4, 3 * ref_err.max()) and err.mean() <= max(1e-6, 2 * ref_err.mean())
  # Baseline: the depth channels of the same hand-off into the Baseline module
  base, _, _, _, _, _ = _tiny_net('Baseline')
  out_b, st_b = base(frames.to(DEV), return_stages=True)
  assert torch.equal(st_b['fusion_input'], HG.disp2depth_frames_gpu(st_b['disp'], st_b['conf'], depth_only=True))
  with torch.no_grad():
    want_b = base.fusion([st_b['fusion_input'][:, p:p + 1] for p in range(6)])
  assert torch.equal(out_b, want_b)


@pytest.mark.gpu
def test_full_size_frame_eager_and_replayed():
  from mode_hip import no_vendor
  from mode_hip.graph_step import GraphedStep
  maxdisp, H, W, sd = _disparity_state('model_wc_full.npz')
  assert (maxdisp, H, W) == (192, 1024, 512)
  net = models.ModeMultiView(maxdisp, 1000., H, W)
  net.disparity.load_state_dict(sd)
  net.fusion.load_state_dict(recipe.recipe_state(recipe.load_manifest('manifest_mode_fusion.json'), 101))
  net = net.to(DEV).eval()
  frames, _, _ = _frames(1, 1024, 512, 102)
  frames = frames.to(DEV)
  with no_vendor.no_vendor_arithmetic() as guard:
    eager, st = net(frames, return_stages=True)
  torch.cuda.synchronize()
  assert guard.seen > 0
  assert bool(torch.isfinite(st['disp']).all()) and bool(torch.isfinite(st['fusion_input']).all())
  assert eager.shape == (1, 1, 1024, 512) and bool(torch.isfinite(eager).all())
  assert float(eager.min()) >= 0 and float(eager.max()) <= 1000
  static = frames.clone()
  step = GraphedStep(lambda: net(static), static_inputs=(static,))
  out = step.replay()
  torch.cuda.synchronize()
  assert torch.equal(out, eager)
