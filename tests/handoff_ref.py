"""A differentiable restatement of the multi-view hand-off's DEPTH channels in torch on the CPU (a helper, not a test): the oracle of
tests/test_gpu_handoff_grad.py and tests/test_handoff_grad_host.py.  dtype is a parameter: float64 is the truth, float32 -- the same
code under CPU autograd -- the yardstick an fp32 kernel is measured against.

  pair 12        the sine rule with the float32 column angle phi_l, clipped by masked assignment (the boundary passes the gradient)
  pairs 13, 14   + F.grid_sample(bilinear, border, align_corners=True) on the cached rotation grid
  pairs 23-34    + a gather at a GIVEN winner-index map, r2 = |r1 dir - t| and the cap at 1000

The winners are an input: they come from the forward's z-buffer keys (decode_keys, layout of csrc/geometry_internal.h).  A float64
z-buffer on the CPU cannot serve -- its winners differ from the GPU's at a few pixels (libm)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from utils import geometry as HG

VIEW_PAIRS = ('23', '24', '34')


def inputs(F_, H, W, seed):
  """Disparities as tests/test_gpu_multiview.py draws them: 10 % zeros, 10 % below 1e-2 (depth far beyond the 1000 m clip), the rest up
  to a quarter of the width; a confidence beside them.  CPU tensors."""
  g = torch.Generator().manual_seed(seed)
  disp = torch.rand(F_, 6, H, W, generator=g) * (W / 4)
  u = torch.rand(F_, 6, H, W, generator=g)
  disp[u < 0.1] = 0
  tiny = (u >= 0.1) & (u < 0.2)
  disp[tiny] = torch.rand(int(tiny.sum()), generator=g) * 1e-2
  conf = torch.rand(F_, 6, H, W, generator=g)
  return disp, conf


def decode_keys(keys):
  """keys (..., H, W) int64, the forward's key planes -> (winner (..., H, W) int64: the flat source index, -1 where no source reached
  the target; v (..., H, W) float32: the stored radius).  key = bits(float32 r2) << 32 | lo, lo = 1 << 31 | k or H W - 1 - k."""
  hw = keys.shape[-2] * keys.shape[-1]
  none = keys == -1
  hi = (keys >> 32) & 0xffffffff
  lo = keys & 0xffffffff
  src = torch.where((lo & 0x80000000) != 0, lo & 0x7fffffff, hw - 1 - lo)
  v = torch.from_numpy(hi.numpy().astype(np.uint32).view(np.float32))
  return torch.where(none, torch.full_like(src, -1), src), torch.where(none, torch.zeros_like(v), v)


def phi_l(W, dtype):
  """The float32 column angle of geom::sine_rule_depth, as values of `dtype`."""
  start = 0.5 * math.pi - (0.5 * math.pi / W)
  return torch.from_numpy((start + np.arange(W, dtype=np.float64) * (-(math.pi / W))).astype(np.float32)).to(dtype)


def sine_rule_raw(disp, baseline, dtype):
  """The unclipped sine-rule depth of disp (..., H, W) (any value where disp == 0)."""
  W = disp.shape[-1]
  pl = phi_l(W, dtype)
  d = torch.where(disp == 0, torch.ones_like(disp), disp)
  phi_r = d * torch.tensor(math.pi, dtype=dtype) / W + pl
  return torch.tensor(float(baseline), dtype=dtype) * torch.sin(torch.tensor(0.5 * math.pi, dtype=dtype) - phi_r) / torch.sin(phi_r - pl)


def sine_rule(disp, baseline, dtype):
  """The clipped depth: 1000 where disp == 0, and the values strictly outside [0, 1000] assigned 1000 / 0 (masked assignment: 0 and 1000
  themselves pass the gradient).  The pixels that pass none are evaluated at a harmless disparity, so that autograd never forms
  0 * inf at a disparity whose float32 depth overflows."""
  with torch.no_grad():
    raw0 = sine_rule_raw(disp, baseline, dtype)
    live = (disp != 0) & (raw0 >= 0) & (raw0 <= 1000)
    fixed = torch.where((disp != 0) & (raw0 < 0), torch.zeros((), dtype=dtype), torch.tensor(1000.0, dtype=dtype))
  raw = sine_rule_raw(torch.where(live, disp, torch.ones_like(disp)), baseline, dtype)
  return torch.where(live, raw, fixed)


def slope(disp, baseline):
  """S(d, j) in float64: -(pi / W) baseline cos(phi_l) / sin^2(d pi / W) where d != 0 and 0 <= raw <= 1000, else 0."""
  disp = disp.double()
  W = disp.shape[-1]
  raw = sine_rule_raw(disp, baseline, torch.float64)
  d = torch.where(disp == 0, torch.ones_like(disp), disp)
  s = -(math.pi / W) * float(baseline) * torch.cos(phi_l(W, torch.float64)) / torch.sin(d * math.pi / W) ** 2
  return torch.where((disp != 0) & (raw >= 0) & (raw <= 1000), s, torch.zeros_like(s))


def near_kink(disp, baseline, rel=1e-3):
  """Pixels whose float64 raw depth lies within `rel` relative of 1000 or within `rel` of 0: either side of the clip may be taken."""
  raw = sine_rule_raw(disp.double(), baseline, torch.float64)
  return (disp != 0) & (((raw - 1000).abs() <= rel * 1000) | (raw.abs() <= rel))


def trig(H, W, dtype):
  """sin phi[W], cos phi[W], sin theta[H], cos theta[H]: the float32 table of the kernels, as values of `dtype`."""
  theta, phi = HG._ranges(H, W)
  theta, phi = theta.astype(np.float32), phi.astype(np.float32)
  return [torch.from_numpy(a.astype(np.float32)).to(dtype) for a in (np.sin(phi), np.cos(phi), np.sin(theta), np.cos(theta))]


def rot_grid(H, W, pair):
  return HG._rotate_grid(H, W, float(HG._ROT_PITCH[pair]), 0.0, 0.0, 'cpu')  # (1, H, W, 2) float32


def view_depth(depth, winner, pair, dtype):
  """depth (H, W) of the source view, winner (H, W) int64 -> the view-transformed depth: r2 of the winner, 0 where there is none,
  capped at 1000 by masked assignment."""
  H, W = depth.shape
  y0, z0, x0, _, _, _ = HG._VIEW_POSES[pair]
  t = [torch.tensor(float(c), dtype=dtype) for c in (x0, y0, z0)]
  sp, cp, st, ct = trig(H, W, dtype)
  w = winner.clamp(min=0).reshape(-1)
  i, j = w // W, w % W
  r1 = depth.reshape(-1)[w]
  rc = r1 * cp[j]
  ax, ay, az = r1 * sp[j] - t[0], rc * st[i] - t[1], rc * ct[i] - t[2]
  r2 = torch.sqrt(ax * ax + ay * ay + az * az).reshape(H, W)
  r2 = torch.where(r2 > 1000, torch.tensor(1000.0, dtype=dtype), r2)
  return torch.where(winner < 0, torch.zeros((), dtype=dtype), r2)


def handoff_depth(disp, winners, dbname='Deep360', dtype=torch.float64):
  """disp (F, 6, H, W) of `dtype` (a leaf that requires a gradient, for instance), winners (F, 3, H, W) int64 -> depth (F, 6, H, W)."""
  F_, _, H, W = disp.shape
  base = HG._baselines(dbname)
  frames = []
  for f in range(F_):
    planes = [sine_rule(disp[f, 0], base[0], dtype)]
    for p, pair in ((1, '13'), (2, '14')):
      src = sine_rule(disp[f, p], base[p], dtype)
      planes.append(F.grid_sample(src[None, None], rot_grid(H, W, pair).to(dtype), mode='bilinear', padding_mode='border', align_corners=True)[0, 0])
    for v, pair in enumerate(VIEW_PAIRS):
      planes.append(view_depth(sine_rule(disp[f, 3 + v], base[3 + v], dtype), winners[f, v], pair, dtype))
    frames.append(torch.stack(planes))
  return torch.stack(frames)


def gradient(disp, winners, gout, dbname='Deep360', dtype=torch.float64):
  """d sum(handoff_depth * gout) / d disp by CPU autograd in `dtype`; gout (F, 6, H, W)."""
  d = disp.detach().to(dtype).requires_grad_(True)
  out = handoff_depth(d, winners, dbname, dtype)
  g, = torch.autograd.grad(out, d, gout.to(dtype))
  return g


def rotation_adjoint_abs(gout, pair):
  """sum_k |w_k gout[t_k]| per source pixel of one rotated plane, in float64 (the bilinear weights are not negative)."""
  H, W = gout.shape
  x = torch.zeros(1, 1, H, W, dtype=torch.float64, requires_grad=True)
  y = F.grid_sample(x, rot_grid(H, W, pair).double(), mode='bilinear', padding_mode='border', align_corners=True)
  g, = torch.autograd.grad(y, x, gout.double().abs()[None, None])
  return g[0, 0]
