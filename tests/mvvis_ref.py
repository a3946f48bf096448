"""The z-buffer visibility of DESIGN 28 (HF.mv_visibility, csrc/mv_visibility.hip; include/mode_hip_mvvis.h has the definition) restated
in float64 with torch on the CPU, the masked multi-view loss restated around tests/mvphoto_ref.py's pieces, and the cases and the scene
its tests share.

    Y, rho, u, v, valid  as tests/mvphoto_ref.py (project), in float64
    landing pixel        x = floor(u + 1/2), y = floor(v + 1/2) mod H of a valid (f, s, h, w)
    z(f, s, y, x)        the minimum of rho over the valid pixels of frame f that land on (y, x) in source s, +inf if none does
    zmin                 z at the landing pixel (radius 0), or the minimum of z over its 3 x 3 neighbourhood, rows modulo H and
                         columns clipped to 0 .. W - 1 (radius 1)
    vis(f, s, h, w)      1 iff valid and rho <= (1 + tol) zmin
    zbuf                 z rounded to float32
    masked loss          mvphoto_ref.mv_loss with `valid for s` replaced by `valid for s and vis(f, s, h, w) != 0`"""
import math

import numpy as np
import torch

import mvphoto_ref as M
import mvpose_ref as P

CASES = M.CASES  # (F, H, W, S): every H is even (include/mode_hip_mvvis.h: with odd H and A = I the middle row lands on the +-pi seam)
# Image seeds (mvphoto_ref.make_case) per case, searched (0, 1, ...) for the first at which the conditions of tests/test_mvvis_host.py
# hold for the masked loss: at 136 x 72 the seeds 0 and 1 leave a runner-up 5.5e-6 and 1.2e-5 behind, under 100 float32 errors.
SEEDS = {CASES[0]: 0, CASES[1]: 0, CASES[2]: 0, CASES[3]: 2}
TOLS, RADII = (0.0, 0.05), (0, 1)
NO_WINNER = M.NO_WINNER


def smooth_depth(F, H, W):
  """(F, H, W) float32: D = 3.5 + 1.2 sin(4 pi h / H + 0.3 + f) cos(3 pi w / W) + 0.8 cos(10 pi h / H + 0.4 w + 0.7 f), in [1.5, 5.5].
  (A random depth map is mostly self-occluding and tests little.)"""
  f = torch.arange(F, dtype=torch.float64).view(F, 1, 1)
  h = torch.arange(H, dtype=torch.float64).view(1, H, 1)
  w = torch.arange(W, dtype=torch.float64).view(1, 1, W)
  D = 3.5 + 1.2 * torch.sin(4 * math.pi * h / H + 0.3 + f) * torch.cos(3 * math.pi * w / W) + 0.8 * torch.cos(10 * math.pi * h / H + 0.4 * w + 0.7 * f)
  return D.float()


def ranges(depth, pose):
  """-> (rho, u, v, valid) of one source, float64: mvphoto_ref.project and, by its own operations, the range it keeps to itself."""
  F, H, W = depth.shape
  u, v, valid = M.project(depth, pose)
  Pm = torch.as_tensor(np.asarray(pose, dtype=np.float64).reshape(3, 4))
  D = depth.double()
  Ds = torch.where(torch.isfinite(D) & (D > 0), D, torch.ones_like(D))
  Y = Ds.unsqueeze(-1) * (M.directions(H, W) @ Pm[:, :3].T) + Pm[:, 3]
  return Y.norm(dim=-1), u.detach(), v.detach(), valid


def neighbourhood_min(z):
  """z (..., H, W) -> the minimum over the 3 x 3 neighbourhood, rows modulo H, columns clipped."""
  rows = torch.minimum(z, torch.minimum(torch.roll(z, 1, -2), torch.roll(z, -1, -2)))
  inf = torch.full_like(rows[..., :1], float('inf'))
  return torch.minimum(rows, torch.minimum(torch.cat([inf, rows[..., :-1]], -1), torch.cat([rows[..., 1:], inf], -1)))


def visibility(depth, poses, tol=0.05, radius=0):
  """depth (F, H, W) any float dtype, poses (S, 12) -> dict: vis (F, S, H, W) uint8, zbuf (F, S, H, W) float32, and in float64 / long
  z, zmin (per reference pixel, +inf where invalid), rho, u, v, valid, at (the landing index y W + x, -1 where invalid)."""
  assert radius in (0, 1) and tol >= 0
  F, H, W = depth.shape
  poses = np.asarray(poses, dtype=np.float64).reshape(-1, 12)
  out = {k: [] for k in ('vis', 'z', 'zmin', 'rho', 'u', 'v', 'valid', 'at')}
  for pose in poses:
    rho, u, v, valid = ranges(depth, pose)
    x = torch.floor(u + 0.5).long()
    y = torch.remainder(torch.floor(v + 0.5).long(), H)
    at = torch.where(valid, y * W + x, torch.zeros_like(x))
    key = torch.where(valid, rho, torch.full_like(rho, float('inf')))
    z = torch.full((F, H * W), float('inf'), dtype=torch.float64).scatter_reduce(1, at.reshape(F, -1), key.reshape(F, -1), 'amin').reshape(F, H, W)
    zn = neighbourhood_min(z) if radius else z
    zmin = torch.where(valid, zn.reshape(F, -1).gather(1, at.reshape(F, -1)).reshape(F, H, W), torch.full_like(rho, float('inf')))
    vis = valid & (rho <= (1.0 + tol) * zmin)
    for k, t in (('vis', vis.to(torch.uint8)), ('z', z), ('zmin', zmin), ('rho', rho), ('u', u), ('v', v), ('valid', valid),
                 ('at', torch.where(valid, at, torch.full_like(at, -1)))):
      out[k].append(t)
  out = {k: torch.stack(t, 1) for k, t in out.items()}
  out['zbuf'] = out['z'].float()
  return out


# ------------------------------------------------------------------------------------------------------------ the masked loss
def mv_loss(ref, src, depth, poses, masks, alpha=0.85, lam=0.1, beta=1.0, mean=None, std=None):
  """mvphoto_ref.mv_loss around the same pieces (warp, pe_map, smoothness) with one change: a pixel is valid for source s iff it is
  valid there and masks[f, s, h, w] != 0.  masks (F, S, H, W), or None for none.  poses: (S, 12) numpy, or a float64 tensor for
  autograd into it (then the warp is mvpose_ref's, mvphoto_ref's operation for operation).  -> (loss, info) as there."""
  dt = depth.dtype
  warp = P.warp if torch.is_tensor(poses) else M.warp
  mean = torch.tensor(M.IMAGENET['mean'] if mean is None else mean, dtype=dt).view(1, 3, 1, 1)
  std = torch.tensor(M.IMAGENET['std'] if std is None else std, dtype=dt).view(1, 3, 1, 1)
  L = ref.to(dt) * std + mean
  F, S, _, H, W = src.shape
  best, idx = None, torch.full((F, H, W - 2), NO_WINNER, dtype=torch.long)
  pes, us, vs, valids = [], [], [], []
  for s in range(S):
    Ih, valid, u, v = warp(src[:, s].to(dt) * std + mean, depth, poses[s])[:4]
    if masks is not None:
      valid = valid & (masks[:, s] != 0)
    pe, wvalid = M.pe_map(L, Ih, valid, alpha)
    better = wvalid & ((idx == NO_WINNER) | (pe.detach() < (best.detach() if best is not None else pe.detach())))
    best = torch.where(better, pe, best if best is not None else torch.zeros_like(pe))
    idx = torch.where(better, torch.full_like(idx, s), idx)
    pes.append(torch.where(wvalid, pe.detach(), torch.full_like(pe, float('inf')).detach()))
    us.append(u.detach())
    vs.append(v.detach())
    valids.append(valid)
  has = idx != NO_WINNER
  n = int(has.sum())
  photo = torch.where(has, best, torch.zeros_like(best)).sum() / max(n, 1)
  smooth = M.smoothness(L, depth, beta)
  loss = photo + lam * smooth if lam != 0 else photo
  win = torch.full((F, H, W), NO_WINNER, dtype=torch.uint8)
  win[..., 1:-1] = idx.to(torch.uint8)
  return loss, {'N': n, 'win': win, 'photo': photo.detach(), 'smooth': smooth.detach(), 'pe': torch.stack(pes), 'u': torch.stack(us),
                'v': torch.stack(vs), 'valid': torch.stack(valids)}


def evaluate(ref, src, depth, poses, masks, dtype, **kw):
  """-> (loss, info, gdepth) of the masked restatement in `dtype`."""
  d = depth.detach().clone().to(dtype).requires_grad_(True)
  loss, info = mv_loss(ref, src, d, poses, masks, **kw)
  g = torch.autograd.grad(loss, d, allow_unused=True)[0] if loss.requires_grad else None
  return loss.detach(), info, torch.zeros_like(d) if g is None else g


def evaluate_poses(ref, src, depth, poses, masks, dtype, **kw):
  """-> (loss, info, gposes (S, 12) float64) of the masked restatement in `dtype` (the geometry and the poses are float64 in both)."""
  pt = torch.as_tensor(np.asarray(poses, dtype=np.float64)).reshape(-1, 12).clone().requires_grad_(True)
  loss, info = mv_loss(ref, src, depth.detach().to(dtype), pt, masks, **kw)
  g = torch.autograd.grad(loss, pt, allow_unused=True)[0] if loss.requires_grad else None
  return loss.detach(), info, torch.zeros_like(pt) if g is None else g


# ---------------------------------------------------------------------------------------------------------------- the cases
def make_case(F, H, W, S):
  """mvphoto_ref.make_case's images (seed: SEEDS) and Deep360's first S default sources, with the smooth depth."""
  ref, src, _, poses = M.make_case(F, H, W, S, seed=SEEDS.get((F, H, W, S), 0))
  return ref, src, smooth_depth(F, H, W), poses


POSE_CASE = CASES[0]  # the case of the gradient to the poses: generic (perturbed) poses, mvpose_ref's for the same shape


def make_pose_case():
  ref, src, depth, _ = make_case(*POSE_CASE)
  return ref, src, depth, P.perturbed_poses(POSE_CASE[3], P.SEEDS[POSE_CASE])


_cache = {}


def _shared(key, fn):
  if key not in _cache:
    _cache[key] = fn()
  return _cache[key]


def reference_visibility(case, tol=0.05, radius=0):
  """visibility() of a case, computed once per (case, tol, radius) and shared; not to be changed."""
  return _shared(('vis', case, tol, radius), lambda: visibility(make_case(*case)[2], make_case(*case)[3], tol, radius))


def reference(case, dtype, **kw):
  """(loss, info, gdepth) of the masked loss of a case with the masks of the defaults (tol 0.05, radius 0), shared."""
  def run():
    ref, src, depth, poses = make_case(*case)
    return evaluate(ref, src, depth, poses, reference_visibility(case)['vis'], dtype, **kw)
  return _shared(('loss', case, dtype, tuple(sorted(kw.items()))), run)


def reference_poses(dtype):
  """(loss, info, gposes, masks) of the pose case, shared."""
  def run():
    ref, src, depth, poses = make_pose_case()
    masks = visibility(depth, poses)['vis']
    return evaluate_poses(ref, src, depth, poses, masks, dtype) + (masks,)
  return _shared(('poses', dtype), run)


def exactness(depth, poses):
  """What the exact comparisons of the masks rest on, measured on the restatement over TOLS x RADII -> dict(land: the smallest
  distance of a valid u + 1/2 or v + 1/2 from an integer, edge: of a valid u from 0 and W - 1, margin: the smallest
  |rho - (1 + tol) zmin| / rho where the minimum is held by another pixel)."""
  W = depth.shape[-1]
  margin = float('inf')
  for tol in TOLS:
    for radius in RADII:
      r = visibility(depth, poses, tol, radius)
      other = r['valid'] & (r['zmin'] < r['rho'])
      if bool(other.any()):
        margin = min(margin, float(((r['rho'] - (1.0 + tol) * r['zmin']).abs() / r['rho'])[other].min()))
  ok, u, v = r['valid'], r['u'], r['v']
  land = min(float(((x + 0.5) - (x + 0.5).round()).abs()[ok].min()) for x in (u, v))
  edge = float(torch.minimum(u.abs(), (u - (W - 1)).abs())[ok].min())
  return {'land': land, 'edge': edge, 'margin': margin}


def loss_conditions(ref, src, depth, poses, masks, pose_tensor=False):
  """DESIGN 25's conditions for a masked case -> dict(err: the float32 restatement's largest pe error, gap: the smallest gap between
  the best and the second-best pe_s, same: float32 and float64 agree on every win and validity, frac: the share of windows with a
  winner, top: the largest share of the windows that one source wins)."""
  F, S, _, H, W = src.shape
  ev = evaluate_poses if pose_tensor else evaluate
  _, i64, _ = ev(ref, src, depth, poses, masks, torch.float64)
  _, i32, _ = ev(ref, src, depth, poses, masks, torch.float32)
  fin = torch.isfinite(i64['pe'])
  same = torch.equal(fin, torch.isfinite(i32['pe'])) and torch.equal(i32['valid'], i64['valid']) and torch.equal(i32['win'], i64['win'])
  err = float((i32['pe'].double() - i64['pe'])[fin & torch.isfinite(i32['pe'])].abs().max())
  gap = float('inf')
  if S > 1:
    srt = torch.sort(i64['pe'], 0).values
    both = torch.isfinite(srt[1])
    gap = float((srt[1] - srt[0])[both].min()) if bool(both.any()) else gap
  windows = float(F * H * (W - 2))
  return {'err': err, 'gap': gap, 'same': same, 'frac': i64['N'] / windows,
          'top': max(int((i64['win'] == s).sum()) for s in range(S)) / windows}


# ------------------------------------------------------------------------------------------------ a scene with a known answer
OCCLUDER_RADIUS = 0.35
OCCLUDER_CENTRE = (0.9, 0.3, 1.1)


def two_spheres(H=64, W=32):
  """The wall of mvphoto_ref.SPHERE_RADIUS around the common camera and an occluding sphere of radius 0.35 at (0.9, 0.3, 1.1), seen
  from panorama 0 (the reference, at the origin) -> (depth (1, H, W) float64: the analytic range along every viewing direction,
  poses (3, 12): panoramas 1, 3, 5 of Deep360, seen (1, 3, H, W) bool: whether the source's centre sees the surface point).
  The occluder is farther from every source's centre than from the reference's, so its splat has no holes.  A point of the wall is
  hidden iff the segment from it to the source's centre meets the occluder; a point of the occluder iff its outward normal points
  away from that segment."""
  _, _, poses = M.sphere_scene(H, W)
  n = M.directions(H, W)
  c = torch.tensor(OCCLUDER_CENTRE, dtype=torch.float64)
  nc = n @ c
  disc = nc * nc - c @ c + OCCLUDER_RADIUS ** 2
  hit = (disc >= 0) & (nc > 0)
  depth = torch.where(hit, nc - torch.sqrt(disc.clamp(min=0)), torch.full_like(nc, M.SPHERE_RADIUS))
  X = depth.unsqueeze(-1) * n
  seen = []
  for pose in poses:
    Pm = torch.as_tensor(np.asarray(pose, dtype=np.float64).reshape(3, 4))
    centre = -(Pm[:, :3].T @ Pm[:, 3])
    assert float((centre - c).norm()) > float(c.norm())
    d = centre - X  # the segment X + t d, 0 < t < 1
    a, b, cc = (d * d).sum(-1), ((X - c) * d).sum(-1), ((X - c) ** 2).sum(-1) - OCCLUDER_RADIUS ** 2
    q = b * b - a * cc
    root = torch.sqrt(q.clamp(min=0))
    t0, t1 = (-b - root) / a, (-b + root) / a
    blocked = (q > 0) & (t1 > 0) & (t0 < 1)
    facing = (((X - c) / OCCLUDER_RADIUS) * d).sum(-1) > 0
    seen.append(torch.where(hit, facing, ~blocked))
  return depth.unsqueeze(0), poses, torch.stack(seen).unsqueeze(0)
