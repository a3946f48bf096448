"""Host references for the gradient of the confidence path (a helper, not a test): the head's confidence map, the confidence channels
of the multi-view hand-off and the decimation.  CPU torch; dtype is a parameter where a float32 yardstick is needed.

  head          oracle/mode_ref.py (disparity_head, confidence_map) under autograd; the closed form p_d (m_d - conf) gconf; and the
                reference's own expression, three grid_sample(mode='nearest') calls on the probability volume
  hand-off      12: the identity; 13, 14: F.grid_sample(bilinear, border, align_corners=True) on the cached rotation grid; 23, 24, 34: a
                gather at GIVEN winners (the forward's z-buffer keys, tests/handoff_ref.py decode_keys), 0 where a target has none
  decimate2     z = zeros; z[..., ::2, ::2] = g"""
import numpy as np
import torch
import torch.nn.functional as F

import handoff_ref as R
from oracle import mode_ref

HALF_BAND = 1e-3  # predictions this close to a half-integer may round either way: their confidence gradient is left out (gconf = 0 there)


def rand(shape, seed, scale=1.0):
  return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32))


# ------------------------------------------------------------------------------------------------ the head
def confidence_three_grid_samples(pred, prob):
  """The confidence as the reference writes it (models/mode_disparity.py:159-180): the probability volume (B, D, H, W) sampled with
  mode='nearest', border padding and align_corners=True at (w, h, round(pred) + k), k = 0, -1, 1, and the three samples added."""
  B, D, H, W = prob.shape
  r = torch.round(pred).permute(0, 2, 3, 1).unsqueeze(1)  # (B, 1, H, W, 1)
  hh, ww = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
  gh = (hh / (H - 1.0) * 2 - 1).to(prob.dtype)[None, None, :, :, None].expand(B, 1, H, W, 1)
  gw = (ww / (W - 1.0) * 2 - 1).to(prob.dtype)[None, None, :, :, None].expand(B, 1, H, W, 1)
  vol = prob.unsqueeze(1)
  out = 0
  for k in (0.0, -1.0, 1.0):
    gd = (r + k) / (D - 1.0) * 2 - 1
    out = out + F.grid_sample(vol, torch.cat([gw, gh, gd], -1), mode='nearest', padding_mode='border', align_corners=True)
  return out.squeeze(1)


def window_multiplicity(pred, D):
  """m (B, D, H, W): how many of clamp(round(pred) + k, 0, D - 1), k = -1, 0, 1, equal d."""
  r = torch.round(pred)
  d = torch.arange(D, dtype=pred.dtype).view(1, D, 1, 1)
  return sum(((r + k).clamp(0, D - 1) == d).to(pred.dtype) for k in (-1.0, 0.0, 1.0))


def head_reference(logits, gpred, gconf, size, dtype=torch.float64):
  """logits (B, 1, D4, H4, W4), gpred, gconf (B, 1, H, W) -> dict: pred, conf, the gradients of sum(gpred pred) and of sum(gconf conf)
  with respect to the logits (the rounding detached), and `unstable`: the pixels within HALF_BAND of a half-integer."""
  D, H, W = size
  la = logits.detach().to(dtype).requires_grad_(True)
  pred, prob = mode_ref.disparity_head(la, D, H, W, return_prob=True)
  conf = mode_ref.confidence_map(pred.detach(), prob)
  g_pred, = torch.autograd.grad(pred, la, gpred.to(dtype), retain_graph=True)
  g_conf, = torch.autograd.grad(conf, la, gconf.to(dtype))
  p = pred.detach()
  unstable = ((p - torch.floor(p)) - 0.5).abs() <= HALF_BAND
  return dict(pred=p, conf=conf.detach(), g_pred=g_pred, g_conf=g_conf, unstable=unstable)


def masked_gconf(logits, gconf, size):
  """gconf with the pixels zeroed whose float64 prediction lies within HALF_BAND of a half-integer, and the share that was zeroed."""
  D, H, W = size
  with torch.no_grad():
    p = mode_ref.disparity_head(logits.double(), D, H, W)
  unstable = ((p - torch.floor(p)) - 0.5).abs() <= HALF_BAND
  out = gconf.clone()
  out[unstable] = 0
  return out, float(unstable.double().mean())


# ------------------------------------------------------------------------------------------------ the hand-off
def handoff_conf(conf, winners):
  """conf (F, 6, H, W) of any float dtype (a leaf that requires a gradient, for instance), winners (F, 3, H, W) int64 -> the confidence
  channels of the hand-off with q the identity, (F, 6, H, W)."""
  F_, _, H, W = conf.shape
  frames = []
  for f in range(F_):
    planes = [conf[f, 0]]
    for p, pair in ((1, '13'), (2, '14')):
      planes.append(F.grid_sample(conf[f, p][None, None], R.rot_grid(H, W, pair).to(conf.dtype), mode='bilinear', padding_mode='border',
                                  align_corners=True)[0, 0])
    for v in range(3):
      w = winners[f, v]
      picked = conf[f, 3 + v].reshape(-1)[w.clamp(min=0).reshape(-1)].reshape(H, W)
      planes.append(torch.where(w < 0, torch.zeros((), dtype=conf.dtype), picked))
    frames.append(torch.stack(planes))
  return torch.stack(frames)


def handoff_conf_gradient(conf, winners, gout_conf, dtype=torch.float64):
  """d sum(handoff_conf * gout_conf) / d conf by CPU autograd in `dtype`; gout_conf (F, 6, H, W)."""
  c = conf.detach().to(dtype).requires_grad_(True)
  g, = torch.autograd.grad(handoff_conf(c, winners), c, gout_conf.to(dtype))
  return g


def winners_scatter(winners, gout_conf):
  """The exact gradient of the view-transformed pairs: winners (F, 3, H, W), gout_conf (F, 3, H, W) -> (F, 3, H, W) float32 with
  gout_conf[t] at the winner of every target t that has one and +0.0 everywhere else (a source wins at most one target)."""
  F_, _, H, W = winners.shape
  out = torch.zeros(F_, 3, H * W, dtype=gout_conf.dtype)
  for f in range(F_):
    for k in range(3):
      w = winners[f, k].reshape(-1)
      t = (w >= 0).nonzero()[:, 0]
      out[f, k, w[t]] = gout_conf[f, k].reshape(-1)[t]
  return out.view(F_, 3, H, W)


# ------------------------------------------------------------------------------------------------ the decimation
def decimate2_bwd(g, shape):
  z = torch.zeros(tuple(shape), dtype=g.dtype)
  z[..., ::2, ::2] = g
  return z
