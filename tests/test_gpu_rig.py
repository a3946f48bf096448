"""The multi-view hand-off and ModeMultiView on any camera rig (utils.rig, csrc/multiview_rig.hip), on the GPU:
  (a) the forward of any rig is its P single calls, bit for bit
  (b) frames and pairs are independent: a subset's planes are the full rig's
  (c) at CameraRig.deep360() the new entries return the bits of the six-pair entries, forward, keys and all three gradients
  (d) a power-of-two scale of the rig scales depth and gradient exactly
  (e) the gradient of poses that no table holds, against float64 autograd on the host
  (f) ModeMultiView(rig=) end to end"""
import functools
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import handoff_ref as R
import recipe
import rig_ref as RR
import test_gpu_handoff_grad as G  # BAND, FLOOR, TINY and the exclusion cap: the measure of the Deep360 rotations
import test_gpu_multiview as M

import models
from dataloader import gpu_ingest
from models import mode_multiview
from utils import geometry as HG
from utils.rig import CameraRig, PairPose

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RIGS = RR.rigs()
SIZES = [(64, 32), (40, 24)]
bits = lambda t: t.view(torch.int32)


# ------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize('size', SIZES, ids=['64x32', '40x24'])
@pytest.mark.parametrize('F', [1, 3])
@pytest.mark.parametrize('name', list(RIGS))
def test_forward_is_the_single_calls_bit_for_bit(name, F, size):
  rig = RIGS[name]
  P, (H, W) = len(rig.pairs), size
  disp, conf = RR.inputs(F, P, H, W, 5 + F + H + P, DEV)
  want = RR.single_calls(disp, conf, rig)
  got, keys = HG.disp2depth_frames_gpu(disp, conf, rig=rig, return_keys=True)
  assert got.shape == (F, 2 * P, H, W) and keys.shape == (F, len(rig.of_kind('view')), H, W) and keys.dtype == torch.int64
  for p, pair in enumerate(rig.pairs):
    assert torch.equal(got[:, 2 * p], want[:, 2 * p]), 'depth of pair %s (%s)' % (pair.name, pair.kind)
    assert torch.equal(got[:, 2 * p + 1], want[:, 2 * p + 1]), 'confidence of pair %s (%s)' % (pair.name, pair.kind)
  # the clip and the ordinary range both taken, by every pair: in its output plane, or for a rotated pair -- whose bilinear taps blend
  # the 1000s with their neighbours -- in the mode_disp2depth plane that the rotation samples
  depth = want[:, 0::2]
  for p, pair in enumerate(rig.pairs):
    own = torch.stack([RR.sine_rule_call(disp[f, p], pair) for f in range(F)]) if pair.kind == 'rotate' else depth[:, p]
    assert bool((own == 1000).any()) and bool(((own > 0) & (own < 1000)).any()), 'pair %s (%s)' % (pair.name, pair.kind)
    assert bool(((depth[:, p] > 0) & (depth[:, p] < 1000)).any()), 'pair %s (%s)' % (pair.name, pair.kind)
  assert torch.equal(HG.disp2depth_frames_gpu(disp.view(P * F, 1, H, W), conf.view(P * F, H, W), rig=rig), got)
  png = HG.disp2depth_frames_gpu(disp, conf, rig=rig, conf_png=True)
  assert torch.equal(png, RR.single_calls(disp, conf, rig, conf_png=True))
  assert torch.equal(png[:, 0::2], got[:, 0::2])
  assert torch.equal(HG.disp2depth_frames_gpu(disp, conf, rig=rig, depth_only=True), got[:, 0::2])
  assert HG.disp2depth_frames_gpu(disp[:0], conf[:0], rig=rig).shape == (0, 2 * P, H, W)
  assert torch.equal(HG.disp2depth_frames_gpu(disp, conf, rig=rig), got)  # (a second call: the key planes are refilled)
  # both gradient entries run for this rig (V = 0 and R = 0 included), write every element and are what autograd returns
  gout = torch.randn(got.shape, generator=torch.Generator().manual_seed(3 + P)).to(DEV)
  gdisp, gconf = HG.disp2depth_frames_bwd(disp, gout, keys, rig=rig, conf_grad=True)
  assert torch.equal(bits(HG.disp2depth_frames_bwd(disp, gout, keys, rig=rig)), bits(gdisp))
  d, c = disp.clone().requires_grad_(True), conf.clone().requires_grad_(True)
  agd, agc = torch.autograd.grad(HG.disp2depth_frames_gpu(d, c, rig=rig, conf_grad=True), (d, c), gout)
  assert torch.equal(bits(agd), bits(gdisp)) and torch.equal(bits(agc), bits(gconf))
  assert bool(torch.isfinite(gdisp).all()) and bool((gdisp != 0).any()) and bool((gconf != 0).any())


# ------------------------------------------------------------------------------------------------ (b)
def _all_three(disp, conf, gout, rig):
  out, keys = HG.disp2depth_frames_gpu(disp, conf, rig=rig, return_keys=True)
  gdisp = HG.disp2depth_frames_bwd(disp, gout, keys, rig=rig)
  gfull, gconf = HG.disp2depth_frames_bwd(disp, gout, keys, rig=rig, conf_grad=True)
  assert torch.equal(bits(gfull), bits(gdisp))
  return out, keys, gdisp, gconf


@pytest.mark.parametrize('size', SIZES, ids=['64x32', '40x24'])
def test_frames_and_pairs_are_independent(size):
  H, W = size
  F, full = 2, RIGS['deep360']
  names = ('23', '12', '14')
  sub = full.subset(names)
  disp, conf = RR.inputs(F, 6, H, W, 21 + H, DEV)
  gout = torch.randn(F, 12, H, W, generator=torch.Generator().manual_seed(22 + H)).to(DEV)
  idx = [full.names.index(n) for n in names]
  ch = [c for p in idx for c in (2 * p, 2 * p + 1)]
  out, keys, gdisp, gconf = _all_three(disp, conf, gout, full)
  s_out, s_keys, s_gdisp, s_gconf = _all_three(disp[:, idx].contiguous(), conf[:, idx].contiguous(), gout[:, ch].contiguous(), sub)
  assert torch.equal(bits(s_out), bits(out[:, ch])) and torch.equal(bits(s_gdisp), bits(gdisp[:, idx])) and torch.equal(bits(s_gconf), bits(gconf[:, idx]))
  assert torch.equal(s_keys[:, 0], keys[:, 0])  # pair 23 is the first view pair of both rigs
  # frame 1 a copy of frame 0: both halves identical, and frame 0 of the F = 2 call is the F = 1 call (plane and key-plane offsets)
  d2, c2, g2 = torch.cat((disp[:1], disp[:1])), torch.cat((conf[:1], conf[:1])), torch.cat((gout[:1], gout[:1]))
  one, two = _all_three(disp[:1], conf[:1], gout[:1], full), _all_three(d2, c2, g2, full)
  for a, b in zip(one, two):
    assert torch.equal(b[0], b[1]) and torch.equal(b[:1], a)
  assert bool((gdisp != 0).any()) and bool((gconf != 0).any())


# ------------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize('size', [(1, 64, 32), (3, 64, 32), (2, 40, 24)], ids=['1x64x32', '3x64x32', '2x40x24'])
def test_deep360_rig_is_the_six_pair_entries_bit_for_bit(size):
  F, H, W = size
  rig, rev = RIGS['deep360'], RIGS['reversed']
  disp, conf = RR.inputs(F, 6, H, W, 31 + F + H, DEV)
  gout = torch.randn(F, 12, H, W, generator=torch.Generator().manual_seed(32 + F + H)).to(DEV)
  gd = gout[:, 0::2].contiguous()
  perm = [5, 4, 3, 2, 1, 0]
  perm2 = [c for p in perm for c in (2 * p, 2 * p + 1)]
  for kw in ({}, {'conf_png': True}, {'depth_only': True}):
    old, old_keys = HG.disp2depth_frames_gpu(disp, conf, return_keys=True, **kw)
    new, new_keys = HG.disp2depth_frames_gpu(disp, conf, rig=rig, return_keys=True, **kw)
    assert torch.equal(bits(new), bits(old)) and torch.equal(new_keys, old_keys), kw
    back, back_keys = HG.disp2depth_frames_gpu(disp[:, perm].contiguous(), conf[:, perm].contiguous(), rig=rev, return_keys=True, **kw)
    assert torch.equal(bits(back), bits(old[:, perm if kw.get('depth_only') else perm2])), kw
    assert torch.equal(back_keys, old_keys[:, [2, 1, 0]]), kw
  keys = old_keys
  old_g = HG.disp2depth_frames_bwd(disp, gout, keys)
  old_alone = HG.disp2depth_frames_bwd(disp, gd, keys, depth_only=True)
  old_full = HG.disp2depth_frames_bwd(disp, gout, keys, conf_grad=True)
  assert torch.equal(bits(HG.disp2depth_frames_bwd(disp, gout, keys, rig=rig)), bits(old_g))
  assert torch.equal(bits(HG.disp2depth_frames_bwd(disp, gd, keys, rig=rig, depth_only=True)), bits(old_alone))
  new_full = HG.disp2depth_frames_bwd(disp, gout, keys, rig=rig, conf_grad=True)
  assert torch.equal(bits(new_full[0]), bits(old_full[0])) and torch.equal(bits(new_full[1]), bits(old_full[1]))
  assert bool((old_g != 0).any()) and bool((old_full[1] != 0).any())
  # the reversed rig: the gradient of every kind at every slot
  rd, rk = disp[:, perm].contiguous(), keys[:, [2, 1, 0]].contiguous()
  assert torch.equal(bits(HG.disp2depth_frames_bwd(rd, gout[:, perm2].contiguous(), rk, rig=rev)), bits(old_g[:, perm]))
  assert torch.equal(bits(HG.disp2depth_frames_bwd(rd, gd[:, perm].contiguous(), rk, rig=rev, depth_only=True)), bits(old_g[:, perm]))
  rev_full = HG.disp2depth_frames_bwd(rd, gout[:, perm2].contiguous(), rk, rig=rev, conf_grad=True)
  assert torch.equal(bits(rev_full[0]), bits(old_full[0][:, perm])) and torch.equal(bits(rev_full[1]), bits(old_full[1][:, perm]))
  # and through autograd, for both inputs
  d, c = disp.clone().requires_grad_(True), conf.clone().requires_grad_(True)
  out = HG.disp2depth_frames_gpu(d, c, rig=rig, conf_grad=True)
  agd, agc = torch.autograd.grad(out, (d, c), gout)
  assert torch.equal(bits(agd), bits(old_full[0])) and torch.equal(bits(agc), bits(old_full[1]))
  d = disp.clone().requires_grad_(True)
  agd, agc = torch.autograd.grad(HG.disp2depth_frames_gpu(d, c, rig=rig), (d, c), gout, allow_unused=True)
  assert agc is None and torch.equal(bits(agd), bits(old_g))
  with pytest.raises(ValueError, match='conf_png'):
    HG.disp2depth_frames_gpu(disp, conf, rig=rig, conf_png=True, conf_grad=True)


# ------------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize('size', SIZES, ids=['64x32', '40x24'])
def test_scale_covariance(size):
  """A power-of-two scale s of every baseline and translation commutes exactly with every operation of sine_rule_depth (a product by
  the baseline, clips that are not reached), project_pixel (contraction off: products and sums of scaled terms, angles of ratios),
  zkey / resolve_key (a scaled radius keeps its order and its rounding) and sine_rule_slope (a product by the baseline)."""
  H, W = size
  F, s = 2, 0.5
  g = torch.Generator().manual_seed(41 + H)
  disp = (W / 64 + torch.rand(F, 6, H, W, generator=g) * (W / 4 - W / 64)).to(DEV)  # no zeros, nothing near the 1000 clip: 1 / sin(pi / 64) ~ 20
  conf = torch.rand(F, 6, H, W, generator=g).to(DEV)
  gout = torch.randn(F, 12, H, W, generator=g).to(DEV)
  unit, half = RIGS['deep360'], CameraRig.square(s)
  o1, k1 = HG.disp2depth_frames_gpu(disp, conf, rig=unit, return_keys=True)
  o2, k2 = HG.disp2depth_frames_gpu(disp, conf, rig=half, return_keys=True)
  assert float(o1[:, 0::2].max()) < 1000
  assert torch.equal(bits(o2[:, 0::2]), bits(s * o1[:, 0::2])), 'depth'
  assert torch.equal(bits(o2[:, 1::2]), bits(o1[:, 1::2])), 'confidence'
  g1 = HG.disp2depth_frames_bwd(disp, gout, k1, rig=unit)
  g2 = HG.disp2depth_frames_bwd(disp, gout, k2, rig=half)
  assert bool((g1 != 0).any()) and torch.equal(bits(g2), bits(s * g1)), 'gdisp'
  # dbname='other' takes the baselines of a square of side 0.6 sqrt 2 but keeps the unit square's translations: the rig that is
  # consistent agrees with it where no translation enters (to the float32 rounding of the baseline) and differs where one does
  other = HG.disp2depth_frames_gpu(disp, conf, 'other')
  cons = HG.disp2depth_frames_gpu(disp, conf, rig=CameraRig.square(0.6 * math.sqrt(2)))
  for p in range(3):
    assert int((bits(other[:, 2 * p].contiguous()) - bits(cons[:, 2 * p].contiguous())).abs().max()) <= 1, HG.PAIRS[p]  # 1 ulp (depths are >= 0)
    assert torch.equal(other[:, 2 * p + 1], cons[:, 2 * p + 1])
  for p in range(3, 6):
    assert float((other[:, 2 * p] - cons[:, 2 * p]).abs().max()) > 1e-2, HG.PAIRS[p]


# ------------------------------------------------------------------------------------------------ (e)
def _free_grid(H, W, dtype):
  return HG._rotate_grid(H, W, *RR.FREE_ROTATE.pose, 'cpu').to(dtype)  # (1, H, W, 2)


def _free_view_depth(depth, winner, dtype):
  """handoff_ref.view_depth with the translation of RR.FREE_VIEW."""
  H, W = depth.shape
  y0, z0, x0 = RR.FREE_VIEW.pose[:3]
  t = [torch.tensor(float(c), dtype=dtype) for c in (x0, y0, z0)]
  sp, cp, st, ct = R.trig(H, W, dtype)
  w = winner.clamp(min=0).reshape(-1)
  i, j = w // W, w % W
  r1 = depth.reshape(-1)[w]
  rc = r1 * cp[j]
  ax, ay, az = r1 * sp[j] - t[0], rc * st[i] - t[1], rc * ct[i] - t[2]
  r2 = torch.sqrt(ax * ax + ay * ay + az * az).reshape(H, W)
  r2 = torch.where(r2 > 1000, torch.tensor(1000.0, dtype=dtype), r2)
  return torch.where(winner < 0, torch.zeros((), dtype=dtype), r2)


def _free_gradient(disp, winner, gd, dtype):
  """d sum(depth planes * gd) / d disp of the rig RIGS['free'] (rotate, view) by CPU autograd in `dtype`."""
  d = disp.detach().to(dtype).requires_grad_(True)
  F_, _, H, W = d.shape
  b = RR.FREE_ROTATE.baseline
  frames = []
  for f in range(F_):
    rot = TF.grid_sample(R.sine_rule(d[f, 0], b, dtype)[None, None], _free_grid(H, W, dtype), mode='bilinear', padding_mode='border',
                         align_corners=True)[0, 0]
    frames.append(torch.stack((rot, _free_view_depth(R.sine_rule(d[f, 1], RR.FREE_VIEW.baseline, dtype), winner[f, 0], dtype))))
  g, = torch.autograd.grad(torch.stack(frames), d, gd.to(dtype))
  return g


@functools.lru_cache(maxsize=None)
def _free_case():
  F, H, W = 2, 40, 24
  rig = RIGS['free']
  disp, conf = RR.inputs(F, 2, H, W, 7 + F + H, 'cpu')
  d, c = disp.to(DEV), conf.to(DEV)
  out, keys = HG.disp2depth_frames_gpu(d, c, rig=rig, return_keys=True)
  winner, v = R.decode_keys(keys.cpu())  # (F, 1, H, W)
  gout = torch.randn(F, 4, H, W, generator=torch.Generator().manual_seed(11 + F + H))
  gd = gout[:, 0::2].contiguous()
  base = [p.baseline for p in rig.pairs]
  S = torch.stack([R.slope(disp[:, p], base[p]) for p in range(2)], 1)
  kink = torch.stack([R.near_kink(disp[:, p], base[p], G.BAND) for p in range(2)], 1)
  den = torch.zeros(F, 2, H, W, dtype=torch.float64)
  won = torch.zeros(F, H * W, dtype=torch.bool)
  capped, near_cap = torch.zeros_like(won), torch.zeros_like(won)
  for f in range(F):
    x = torch.zeros(1, 1, H, W, dtype=torch.float64, requires_grad=True)
    y = TF.grid_sample(x, _free_grid(H, W, torch.float64), mode='bilinear', padding_mode='border', align_corners=True)
    adj, = torch.autograd.grad(y, x, gd[f, 0].double().abs()[None, None])
    den[f, 0] = S[f, 0].abs() * adj[0, 0]  # |S| sum_k |w_k gout_tk|, as for pairs 13 and 14
    t = (winner[f, 0].reshape(-1) >= 0).nonzero()[:, 0]
    s = winner[f, 0].reshape(-1)[t]
    assert s.unique().numel() == s.numel()  # a source wins at most one target
    won[f, s] = True
    capped[f, s] = v[f, 0].reshape(-1)[t] > 1000
    near_cap[f, s] = (v[f, 0].reshape(-1)[t].double() - 1000).abs() <= G.BAND * 1000
    den[f, 1].view(-1)[s] = gd[f, 1].reshape(-1)[t].double().abs() * S[f, 1].reshape(-1)[s].abs()
  skip = kink.clone()
  skip[:, 1] |= near_cap.view(F, H, W) & (S[:, 1] != 0)
  return dict(disp=disp, d=d, keys=keys, gout=gout, gd=gd, S=S, kink=kink, den=den, won=won.view(F, H, W), capped=capped.view(F, H, W),
              skip=skip, winner=winner, ref64=_free_gradient(disp, winner, gd, torch.float64),
              ref32=_free_gradient(disp, winner, gd, torch.float32).double())


def test_gradient_of_unpinned_poses_against_float64():
  """The measure, the bounds and the exclusion of tests/test_gpu_handoff_grad.py (its score / assert_within_the_yardstick, written
  for two planes): the error of an element in units of |S| sum_k |w_k gout_tk| (rotate) or |gout_t| |S| (view), its mean at most
  twice and its maximum at most three times what float32 autograd of the same functions achieves, pixels within BAND of a clip
  boundary left out, at most 0.5 % of a plane."""
  z = _free_case()
  rig = RIGS['free']
  got = HG.disp2depth_frames_bwd(z['d'], z['gout'].to(DEV), z['keys'], rig=rig).cpu()
  assert got.shape == z['disp'].shape and got.dtype == torch.float32
  alone = HG.disp2depth_frames_bwd(z['d'], z['gd'].to(DEV), z['keys'], rig=rig, depth_only=True).cpu()
  assert torch.equal(bits(alone), bits(got))
  left_out = z['skip'].double().mean((2, 3))
  assert float(left_out.max()) <= 0.005, 'more than 0.5 %% of a plane left out of the scoring: %s' % left_out
  F = got.shape[0]
  for name, t in (('kernel', got), ('float32 autograd', z['ref32'])):
    err = (t.double() - z['ref64']).abs() / (z['den'] + G.TINY)
    z[name] = {(f, p): (float(err[f, p][~z['skip'][f, p]].mean()), float(err[f, p][~z['skip'][f, p]].max())) for f in range(F) for p in range(2)}
  for key in sorted(z['kernel']):
    (m, x), (ym, yx) = z['kernel'][key], z['float32 autograd'][key]
    print('frame %d pair %s: kernel mean %.3e max %.3e; float32 autograd mean %.3e max %.3e' % (key[0], rig.pairs[key[1]].name, m, x, ym, yx))
    assert m <= max(2 * ym, G.FLOOR) and x <= max(3 * yx, G.FLOOR), (key, m, x, ym, yx)
  assert bool((z['S'] == 0).any()) and bool((z['S'] != 0).any()) and bool(z['won'].any()) and bool((z['winner'] < 0).any())


def test_view_pair_gradient_is_the_winners_alone():
  """As test_gpu_handoff_grad.test_structural_zeros_are_exact, for the free poses."""
  z = _free_case()
  g = HG.disp2depth_frames_bwd(z['d'], z['gout'].to(DEV), z['keys'], rig=RIGS['free']).cpu()
  b = bits(g)
  assert not bool(torch.isnan(g).any())
  sure = ~z['kink']
  zero = (z['disp'] == 0) | ((z['S'] == 0) & sure)
  zero[:, 1] |= ~z['won'] | z['capped']
  assert bool((z['disp'] == 0).any()) and bool(((z['S'] == 0) & (z['disp'] != 0)).any()) and bool(zero[:, 1].any())
  assert bool((b[zero] == 0).all()), 'a structural zero is not +0.0: %d of %d' % (int((b[zero] != 0).sum()), int(zero.sum()))
  live = z['won'] & ~z['capped'] & (z['S'][:, 1] != 0)
  assert int(live.sum()) > 0 and int(((g[:, 1] != 0) & sure[:, 1]).sum()) == int((live & sure[:, 1]).sum())
  if not bool((z['kink'][:, 1] & z['won']).any()):
    assert int((g[:, 1] != 0).sum()) == int(live.sum())


# ------------------------------------------------------------------------------------------------ (f)
def _tiny_net(rig, **kw):
  """tests/test_gpu_multiview._tiny_net for a rig: model_wc_tiny's disparity state; the fusion network's recipe state with fusion_tiny's
  seed over the module's own shapes (its first two layers have other shapes than the fixture's manifest)."""
  maxdisp, H, W, sd = M._disparity_state('model_wc_tiny.npz')
  zf = np.load(os.path.join(recipe.HERE, 'fusion_tiny.npz'))
  cfg = zf['cfg']
  maxdepth, seed, channels = float(cfg[0]), int(cfg[4]), tuple(int(c) for c in cfg[5:])
  assert (maxdisp, H, W) == (16, 64, 32) and channels == (8, 16, 32, 64)
  net = models.ModeMultiView(maxdisp, maxdepth, H, W, channels=channels, rig=rig, **kw)
  net.disparity.load_state_dict(sd)
  net.fusion.load_state_dict(recipe.recipe_state([(k, tuple(v.shape)) for k, v in net.fusion.state_dict().items()], seed))
  return net.to(DEV).eval(), maxdepth, H, W


def _u8_frames(F, n, H, W, seed):
  return torch.randint(0, 256, (F, n, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _host_normalised(frames_u8):
  """(F, n, H, W, 3) uint8 -> (F, n, 3, H, W) float32 as the host transform normalises a panorama (the table of the 256 byte values)."""
  from dataloader import preprocess
  lut = preprocess.norm_table().to(frames_u8.device)  # (256, 3)
  x = frames_u8.long()
  return torch.stack([lut[x[..., ch], ch] for ch in range(3)], 2).contiguous()


def _grads(module):
  return {k: (None if p.grad is None else p.grad.clone()) for k, p in module.named_parameters()}


def test_ingest_of_a_rig_is_the_float_split():
  for name in ('subset', 'mixed16', 'one_view', 'deep360'):
    rig = RIGS[name]
    P, H, W, F = len(rig.pairs), 16, 8, 2
    u8 = _u8_frames(F, 2 * P, H, W, 90 + P)
    want = mode_multiview.split_frames(_host_normalised(u8), rig)
    got = gpu_ingest.frames_u8_gpu(u8, rig=rig)
    assert got[0].shape == (P * F, 3, H, W) and got[2].shape == (F, 3 * len(rig.rgb), H, W)
    for a, b in zip(got, want):
      assert torch.equal(bits(a.contiguous()), bits(b.contiguous())), name
    left, right, none = gpu_ingest.frames_u8_gpu(u8, want_rgb=False, rig=rig)
    assert none is None and torch.equal(left, want[0]) and torch.equal(right, want[1])
  d = RIGS['deep360']
  u8 = _u8_frames(2, 12, 16, 8, 97)
  for a, b in zip(gpu_ingest.frames_u8_gpu(u8, rig=d), gpu_ingest.frames_u8_gpu(u8)):
    assert torch.equal(a, b)
  params = gpu_ingest.draw_colour_params(24, DEV, generator=torch.Generator().manual_seed(5))
  for a, b in zip(gpu_ingest.frames_u8_gpu(u8, augment=params, rig=d), gpu_ingest.frames_u8_gpu(u8, augment=params)):
    assert torch.equal(a, b)


def test_module_on_three_pairs():
  from mode_hip import no_vendor
  rig = RIGS['subset']  # 12, 13, 23: one pair of each kind, rgb = panoramas 0 and 1
  net, maxdepth, H, W = _tiny_net(rig)
  F, P = 2, 3
  u8 = _u8_frames(F, 2 * P, H, W, 43)
  frames = _host_normalised(u8)
  with no_vendor.no_vendor_arithmetic():
    depth, st = net(frames, return_stages=True)
    depth_u8 = net(u8)
  assert depth.shape == (F, 1, H, W) and torch.equal(bits(depth_u8), bits(depth))
  # stage by stage, by hand
  left, right, rgb = mode_multiview.split_frames(frames, rig)
  with torch.no_grad():
    disp, conf = net.disparity(left, right)
    assert disp.shape == (P * F, 1, H, W) and torch.equal(st['disp'], disp) and torch.equal(st['conf'], conf)
    fi = RR.single_calls(disp.view(F, P, H, W), conf.view(F, P, H, W), rig, conf_png=True)
    assert fi.shape == (F, 6, H, W) and torch.equal(bits(st['fusion_input']), bits(fi))
    assert torch.equal(bits(net.fusion.feature_extraction(fi, rgb)), bits(depth))
  gt = (torch.rand(F, H, W, generator=torch.Generator().manual_seed(44)) * 1.25 * maxdepth).to(DEV)
  erp, rows = net.evaluate(u8, gt)
  assert tuple(erp.shape) == (F, W, H) and rows.shape == (F, 8) and np.isfinite(rows).all()
  # fusion_loss, stage 1 frozen
  net.train()
  net.disparity.eval()
  with no_vendor.no_vendor_arithmetic():
    loss, out = net.fusion_loss(u8, gt)
    loss.backward()
  assert loss.dim() == 0 and bool(torch.isfinite(loss)) and tuple(out.shape) == (F, 1, H, W)
  have = _grads(net)
  for k, g in have.items():
    if k.startswith('disparity.'):
      assert g is None, k
    else:
      assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, k
  again, _, _, _ = _tiny_net(rig)
  again.train()
  again.disparity.eval()
  loss2, out2 = again.fusion_loss(frames, gt)
  loss2.backward()
  assert torch.equal(loss2, loss) and torch.equal(out2, out)
  for k, g in _grads(again).items():
    assert (g is None and have[k] is None) or torch.equal(g, have[k]), k


def test_module_fine_tunes_stage_one_through_a_rig():
  from mode_hip import no_vendor
  rig = RIGS['subset']
  net, maxdepth, H, W = _tiny_net(rig, conf_png=False, handoff_grad='full')
  frames = _host_normalised(_u8_frames(1, 6, H, W, 45))
  gt = (torch.rand(1, H, W, generator=torch.Generator().manual_seed(46)) * 1.25 * maxdepth).to(DEV)
  net.train()
  with no_vendor.no_vendor_arithmetic():
    loss, _ = net.fusion_loss(frames, gt)
    loss.backward()
  assert bool(torch.isfinite(loss))
  for k, g in _grads(net).items():
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, k
  depth, _, _, _ = _tiny_net(rig)  # handoff_grad='depth': the depth channels alone
  depth.train()
  loss, _ = depth.fusion_loss(frames, gt)
  loss.backward()
  assert all(g is not None and float(g.abs().max()) > 0 for k, g in _grads(depth).items() if k.startswith('disparity.'))


def test_module_with_the_deep360_rig_is_the_module_without():
  plain, _, _, maxdepth, H, W = M._tiny_net()
  rigged, _, _, _ = _tiny_net(RIGS['deep360'])
  rigged.load_state_dict(plain.state_dict())
  F = 1
  u8 = _u8_frames(F, 12, H, W, 47)
  gt = (torch.rand(F, H, W, generator=torch.Generator().manual_seed(48)) * 1.25 * maxdepth).to(DEV)
  assert torch.equal(bits(rigged(u8)), bits(plain(u8)))
  (e1, r1), (e2, r2) = rigged.evaluate(u8, gt), plain.evaluate(u8, gt)
  assert torch.equal(bits(e1), bits(e2)) and np.array_equal(r1, r2)
  for net in (plain, rigged):
    net.train()
    net.disparity.eval()
  (l1, o1), (l2, o2) = rigged.fusion_loss(u8, gt), plain.fusion_loss(u8, gt)
  assert torch.equal(l1, l2) and torch.equal(bits(o1), bits(o2))


def test_module_on_one_view_pair():
  """P = 1, kind 'view', rgb = (0,): first layers with 2 and 3 input channels."""
  from mode_hip import no_vendor
  rig = CameraRig([RR.FREE_VIEW], (0,))
  net, maxdepth, H, W = _tiny_net(rig)
  fe = net.fusion.feature_extraction
  assert tuple(next(iter(fe.depth_layer1.parameters())).shape) == (8, 2, 3, 3) and tuple(next(iter(fe.rgb_layer1.parameters())).shape) == (8, 3, 3, 3)
  u8 = _u8_frames(2, 2, H, W, 49)
  with no_vendor.no_vendor_arithmetic():
    depth, st = net(u8, return_stages=True)
  assert depth.shape == (2, 1, H, W) and bool(torch.isfinite(depth).all())
  fi = RR.single_calls(st['disp'].view(2, 1, H, W), st['conf'].view(2, 1, H, W), rig, conf_png=True)
  assert torch.equal(bits(st['fusion_input']), bits(fi))
  gt = (torch.rand(2, H, W, generator=torch.Generator().manual_seed(50)) * 1.25 * maxdepth).to(DEV)
  net.train()
  net.disparity.eval()
  with no_vendor.no_vendor_arithmetic():
    loss, _ = net.fusion_loss(u8, gt)
    loss.backward()
  assert all(float(p.grad.abs().max()) > 0 for p in net.fusion.parameters())
