"""The novel-view rendering of DESIGN 29 (HF.mv_render, csrc/mv_render.hip; include/mode_hip_mvrender.h has the definition) restated
with torch on the CPU, the geometry in float64, and the cases and conditions its tests share.

    Y, rho, u, v, valid  as tests/mvvis_ref.py (ranges), in float64; landing pixel x = floor(u + 1/2), y = floor(v + 1/2) mod H
    z(f, t, y, x)        the minimum of rho over the valid pixels that land there, +inf if none does
    owner(f, t, y, x)    the smallest h W + w among the valid pixels that land there with rho == z, -1 if none does
    fill == 0            finite z: DIRECT, zc = z, from = owner; otherwise NONE
    fill == 1            zn = min of z over the 3 x 3 neighbourhood (rows modulo H, columns clipped); DIRECT iff z finite and
                         z <= (1 + tol) zn; otherwise FILLED if zn is finite: zc = zn, from = the owner of the first neighbour holding zn
                         (dy = -1, 0, 1 outside, dx = -1, 0, 1 inside); otherwise NONE
    range, index         zc rounded to float32 (+inf for NONE); from (-1 for NONE)
    SPLAT                out(f, t, c, y, x) = image(f, c, from), 0 for NONE
    RESAMPLE             X = A^T (zc n(y, x) - o), r = |X|, u_r, v_r by mvphoto_ref's formulas; if r > 0 and 0 <= u_r <= W - 1 the
                         bilinear value (x0 = min(floor u_r, W - 2), rows floor v_r and + 1 modulo H; t, q rounded to the working dtype,
                         top, bot, then rows) and hit += 4; otherwise SPLAT's value
The working dtype (float64 or float32) is that of t, q and the bilinear alone: float32 is what the kernel computes in, float64 the
reference of the yardstick."""
import math

import numpy as np
import torch

import mvphoto_ref as M
import mvpose_ref as P
import mvvis_ref as V

SPLAT, RESAMPLE = 0, 1
NONE, DIRECT, FILLED, RESAMPLED = 0, 1, 2, 4
TOLS, FILLS = (0.0, 0.05), (0, 1)
# The target poses of every case: the identity twisted by the first T of these rows (omega, tau) (mvpose_ref.twisted).
TW = ((0.01, 0.02, -0.015, 0.10, 0.02, -0.03), (0.05, -0.12, 0.08, -0.04, 0.07, 0.05), (-0.3, 0.2, 0.15, 0.15, -0.1, 0.2))
CASES = M.CASES  # (F, H, W, T) with the smooth depth of mvvis_ref
SPHERES = ('two spheres', 64, 32, 3)
_BIG = 1 << 40


def poses_of(T):
  """(T, 12) float64 numpy: [I | 0] twisted by TW[:T]."""
  eye = torch.eye(3, 4, dtype=torch.float64).reshape(1, 12).repeat(T, 1)
  return np.ascontiguousarray(P.twisted(eye, torch.tensor(TW[:T], dtype=torch.float64)).numpy())


def _shift(a, dy, dx, pad):
  """a (..., H, W) -> b with b[y, x] = a[(y + dy) mod H, x + dx], `pad` where x + dx is outside 0 .. W - 1."""
  b = torch.roll(a, -dy, -2)
  if dx == 0:
    return b
  edge = torch.full_like(b[..., :1], pad)
  return torch.cat([b[..., 1:], edge], -1) if dx > 0 else torch.cat([edge, b[..., :-1]], -1)


def zbuffer(depth, pose):
  """depth (F, H, W), one pose -> dict in float64 / long: z (F, H, W), owner (F, H, W), and per reference pixel rho, u, v, valid, at."""
  F, H, W = depth.shape
  rho, u, v, valid = V.ranges(depth, pose)
  x = torch.floor(u + 0.5).long().clamp(0, W - 1)
  y = torch.remainder(torch.floor(v + 0.5).long(), H)
  at = torch.where(valid, y * W + x, torch.zeros_like(x)).reshape(F, -1)
  key = torch.where(valid, rho, torch.full_like(rho, float('inf'))).reshape(F, -1)
  z = torch.full((F, H * W), float('inf'), dtype=torch.float64).scatter_reduce(1, at, key, 'amin')
  mine = valid.reshape(F, -1) & (key == z.gather(1, at))
  pixel = torch.arange(H * W).expand(F, -1)
  owner = torch.full((F, H * W), _BIG, dtype=torch.long).scatter_reduce(1, at, torch.where(mine, pixel, torch.full_like(pixel, _BIG)), 'amin')
  owner = torch.where(owner == _BIG, torch.full_like(owner, -1), owner)
  return {'z': z.reshape(F, H, W), 'owner': owner.reshape(F, H, W), 'rho': rho, 'u': u, 'v': v, 'valid': valid,
          'at': torch.where(valid, at.reshape(F, H, W), torch.full_like(x, -1))}


def resolve(z, owner, tol, fill):
  """-> (cls, zc, src, zn): the class, the range and the reference pixel of every target pixel; zn the neighbourhood's minimum."""
  inf = torch.full_like(z, float('inf'))
  none = torch.full_like(owner, -1)
  if not fill:
    direct = torch.isfinite(z)
    return direct.long() * DIRECT, torch.where(direct, z, inf), torch.where(direct, owner, none), z
  zn, first = inf, none
  for dy in (-1, 0, 1):
    for dx in (-1, 0, 1):
      zz, oo = _shift(z, dy, dx, float('inf')), _shift(owner, dy, dx, -1)
      better = zz < zn
      zn, first = torch.where(better, zz, zn), torch.where(better, oo, first)
  direct = torch.isfinite(z) & (z <= (1.0 + tol) * zn)
  filled = ~direct & torch.isfinite(zn)
  cls = direct.long() * DIRECT + filled.long() * FILLED
  return cls, torch.where(direct, z, torch.where(filled, zn, inf)), torch.where(direct, owner, torch.where(filled, first, none)), zn


def back_project(zc, seen, pose, H, W):
  """The target pixels' own rays at range zc, back in the reference: -> (u_r, v_r float64, ok: seen, r > 0 and 0 <= u_r <= W - 1)."""
  Pm = torch.as_tensor(np.asarray(pose, dtype=np.float64).reshape(3, 4))
  zs = torch.where(seen, zc, torch.ones_like(zc))
  X = (zs.unsqueeze(-1) * M.directions(H, W) - Pm[:, 3]) @ Pm[:, :3]  # A^T d, row by row
  r = X.norm(dim=-1)
  pos = seen & (r > 0)
  rs = torch.where(pos, r, torch.ones_like(r))
  phi = torch.asin((X[..., 0] / rs).clamp(-1, 1))
  theta = torch.atan2(X[..., 1], X[..., 2])
  u = (math.pi / 2 - phi) * W / math.pi - 0.5
  v = (math.pi - theta) * H / (2.0 * math.pi) - 0.5
  return u, v, pos & (u >= 0) & (u <= W - 1)


def _gather(flat, idx):
  """flat (F, C, HW), idx (F, H, W) long in 0 .. HW - 1 -> (F, C, H, W)."""
  F, C, _ = flat.shape
  return flat.gather(2, idx.reshape(F, 1, -1).expand(F, C, -1)).reshape((F, C) + idx.shape[1:])


def render(image, depth, poses, tol=0.05, fill=1, mode=RESAMPLE, dtype=torch.float64):
  """image (F, C, H, W), depth (F, H, W) any float dtype, poses (T, 12) -> dict: out (F, T, C, H, W) in `dtype`, hit (F, T, H, W) uint8,
  range float32, index int32, and in float64 z, zn, zc, u_r, v_r with ok (resampled) and the list `buffers` of zbuffer() per view."""
  assert fill in (0, 1) and mode in (SPLAT, RESAMPLE) and tol >= 0
  F, C, H, W = image.shape
  flat = image.to(dtype).reshape(F, C, H * W)
  poses = np.asarray(poses, dtype=np.float64).reshape(-1, 12)
  keep = {k: [] for k in ('out', 'hit', 'range', 'index', 'z', 'zn', 'zc', 'u_r', 'v_r', 'ok')}
  buffers = []
  for pose in poses:
    zb = zbuffer(depth, pose)
    buffers.append(zb)
    cls, zc, src, zn = resolve(zb['z'], zb['owner'], tol, fill)
    seen = cls != NONE
    splat = torch.where(seen.unsqueeze(1), _gather(flat, src.clamp(min=0)), torch.zeros((), dtype=dtype))
    u, v, ok = back_project(zc, seen, pose, H, W)
    out = splat
    if mode == RESAMPLE:
      us, vs = torch.where(ok, u, torch.zeros_like(u)), torch.where(ok, v, torch.zeros_like(v))
      x0 = us.floor().clamp(max=W - 2)
      y0 = vs.floor()
      t, q = (us - x0).to(dtype).unsqueeze(1), (vs - y0).to(dtype).unsqueeze(1)
      x0 = x0.long()
      ya, yb = torch.remainder(y0.long(), H), torch.remainder(y0.long() + 1, H)
      top = (1 - t) * _gather(flat, ya * W + x0) + t * _gather(flat, ya * W + x0 + 1)
      bot = (1 - t) * _gather(flat, yb * W + x0) + t * _gather(flat, yb * W + x0 + 1)
      out = torch.where(ok.unsqueeze(1), (1 - q) * top + q * bot, splat)
    else:
      ok = torch.zeros_like(ok)
    for k, t_ in (('out', out), ('hit', (cls + RESAMPLED * ok.long()).to(torch.uint8)), ('range', zc.float()), ('index', src.to(torch.int32)),
                  ('z', zb['z']), ('zn', zn), ('zc', zc), ('u_r', u), ('v_r', v), ('ok', ok)):
      keep[k].append(t_)
  res = {k: torch.stack(t_, 1) for k, t_ in keep.items()}
  res['buffers'] = buffers
  return res


# ---------------------------------------------------------------------------------------------------------------- the cases
def make_case(case):
  """-> (image (F, 3, H, W) float32, depth (F, H, W) float32, poses (T, 12)): mvvis_ref's images with the smooth depth for a case of
  CASES; the wall and its occluder with the sphere scene's reference image for SPHERES."""
  if case == SPHERES:
    _, H, W, T = case
    return M.sphere_scene(H, W)[0].float(), V.two_spheres(H, W)[0].float(), poses_of(T)
  F, H, W, T = case
  return V.make_case(F, H, W, T)[0], V.smooth_depth(F, H, W), poses_of(T)


def channels(image, C):
  """The image with C = 1, 3 or 4 planes: its first, itself, or itself and the mean of its planes."""
  return {1: image[:, :1], 3: image, 4: torch.cat([image, image.mean(1, keepdim=True)], 1)}[C].contiguous()


_cache = {}


def reference(case, tol=0.05, fill=1, mode=RESAMPLE, dtype=torch.float64, C=3):
  """render() of a case, computed once per setting and shared; not to be changed."""
  key = (case, tol, fill, mode, dtype, C)
  if key not in _cache:
    image, depth, poses = make_case(case)
    _cache[key] = render(channels(image, C), depth, poses, tol, fill, mode, dtype)
  return _cache[key]


def _from_integer(x):
  return (x - x.round()).abs()


def exactness(case):
  """What the exact comparisons rest on, measured on the float64 restatement of a case over TOLS x FILLS -> dict:
    land    the smallest distance of a valid u + 1/2 or v + 1/2 from an integer
    edge    the smallest distance of a valid u from 0 and W - 1
    pixel   the smallest relative gap between the smallest and the second rho that land on one target pixel
    near    the smallest relative gap between the smallest and the second key of a 3 x 3 neighbourhood
    margin  the smallest |z - (1 + tol) zn| / z at tol = 0.05 where another pixel holds zn
    redge   the smallest distance of a resampling u_r from 0 and W - 1, rint: of u_r or v_r from an integer"""
  image, depth, poses = make_case(case)
  F, H, W = depth.shape
  out = {k: float('inf') for k in ('land', 'edge', 'pixel', 'near', 'margin', 'redge', 'rint')}
  for pose in poses:
    zb = zbuffer(depth, pose)
    ok = zb['valid']
    out['land'] = min([out['land']] + [float(_from_integer(x + 0.5)[ok].min()) for x in (zb['u'], zb['v'])])
    out['edge'] = min(out['edge'], float(torch.minimum(zb['u'].abs(), (zb['u'] - (W - 1)).abs())[ok].min()))
    for f in range(F):  # the two smallest rho per target pixel
      at, rho = zb['at'][f][ok[f]].numpy(), zb['rho'][f][ok[f]].numpy()
      order = np.lexsort((rho, at))
      at, rho = at[order], rho[order]
      start = np.concatenate([[True], at[1:] != at[:-1]])
      second = np.concatenate([[False], start[:-1] & ~start[1:]])
      if second.any():
        out['pixel'] = min(out['pixel'], float(((rho[second] - rho[np.roll(second, -1)]) / rho[np.roll(second, -1)]).min()))
    nine = torch.sort(torch.stack([_shift(zb['z'], dy, dx, float('inf')) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]), 0).values
    two = torch.isfinite(nine[1])
    out['near'] = min(out['near'], float(((nine[1] - nine[0]) / nine[0])[two].min()))
  for tol in TOLS:
    for fill in FILLS:
      r = render(image, depth, poses, tol, fill, RESAMPLE)
      if fill and tol == 0.05:
        other = torch.isfinite(r['z']) & (r['zn'] < r['z'])
        out['margin'] = min(out['margin'], float(((r['z'] - (1.0 + tol) * r['zn']).abs() / r['z'])[other].min()))
      seen = r['hit'] != NONE
      u, v = r['u_r'], r['v_r']
      out['redge'] = min(out['redge'], float(torch.minimum(u.abs(), (u - (W - 1)).abs())[seen].min()))
      out['rint'] = min([out['rint']] + [float(_from_integer(x)[r['ok']].min()) for x in (u, v)])
  return out
