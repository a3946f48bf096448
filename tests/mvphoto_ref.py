"""The multi-view reprojection loss of DESIGN 25 (HF.mv_photometric_loss, csrc/mv_photometric.hip) restated from its definition as a
torch function on the CPU, in float64 or float32, with autograd into the depth; and the seeded cases and the scene its tests share.

    L, src      = image * std + mean                       ref (F, 3, H, W), src (F, S, 3, H, W); H is Cassini's periodic axis
    n(h, w)     = (sin phi, cos phi sin theta, cos phi cos theta), theta = pi - (h + 1/2) 2 pi / H, phi = pi/2 - (w + 1/2) pi / W
    Y           = depth (A n) + o;  rho = |Y|;  phi' = asin(Y_x / rho);  theta' = atan2(Y_y, Y_z)
    u, v        = (pi/2 - phi') W / pi - 1/2,  (pi - theta') H / (2 pi) - 1/2
    valid       iff depth finite and > 0, rho > 0, 0 <= u <= W - 1
    x0, t       = min(floor(u), W - 2), u - x0;   y0, q = floor(v), v - y0;   rows y0 mod H and (y0 + 1) mod H
    Ih_s        the bilinear value (0 and without a gradient where invalid)
    pe_s        tests/photometric_ref.py's pe between L and Ih_s; a window is valid for s iff its nine pixels are
    win         the smallest s attaining min_s pe_s over the sources whose window is valid, 255 if none is
    photo       sum of the minima / max(N, 1)
    smooth      mean over F H (W - 1) column neighbours of |log D(h, w+1) - log D(h, w)| exp(-beta mean_c |L_c(h, w+1) - L_c(h, w)|) + the
                mean over F H W row neighbours (h + 1 modulo H) of the same; a pair with a depth not finite and > 0 contributes 0
    loss        photo + lam smooth; lam == 0 leaves the smoothness term out altogether

The geometry (u, v) is float64 in both restatements, as in the kernel; the float32 one rounds at t and q, and autograd rounds the slopes
where they meet the float32 bilinear."""
import math

import numpy as np
import torch

import photometric_ref as R

from utils.rig import CameraRig

IMAGENET = R.IMAGENET
CASES = ((2, 40, 24, 3), (1, 64, 32, 1), (1, 70, 37, 2), (1, 136, 72, 3))  # (F, H, W, S)
SEEDS = {CASES[0]: 0, CASES[1]: 0, CASES[2]: 0, CASES[3]: 23}  # chosen so that the conditions of tests/test_mvphoto_host.py hold
NO_WINNER = 255


def deep360_poses(sources=None):
  """(S, 12) float64: the poses of Deep360's default sources (1, 3, 5), or of the panoramas named."""
  rig = CameraRig.deep360()
  sources = rig.default_sources() if sources is None else sources
  return rig.panorama_poses()[list(sources)].reshape(-1, 12)


def directions(H, W):
  """(H, W, 3) float64 viewing directions, angles at pixel centres."""
  theta = (math.pi - (torch.arange(H, dtype=torch.float64) + 0.5) * 2.0 * math.pi / H).view(H, 1)
  phi = (math.pi / 2 - (torch.arange(W, dtype=torch.float64) + 0.5) * math.pi / W).view(1, W)
  return torch.stack([torch.sin(phi).expand(H, W), torch.cos(phi) * torch.sin(theta), torch.cos(phi) * torch.cos(theta)], -1)


def project(depth, pose):
  """depth (F, H, W) any float dtype, pose (12,) -> (u, v (F, H, W) float64 with autograd through depth, valid (F, H, W) bool)."""
  F, H, W = depth.shape
  P = torch.as_tensor(np.asarray(pose, dtype=np.float64).reshape(3, 4))
  D = depth.double()
  good = torch.isfinite(D) & (D > 0)
  Ds = torch.where(good, D, torch.ones_like(D))
  m = directions(H, W) @ P[:, :3].T  # (H, W, 3)
  Y = Ds.unsqueeze(-1) * m + P[:, 3]
  rho = Y.norm(dim=-1)
  ok = good & (rho > 0)
  rs = torch.where(ok, rho, torch.ones_like(rho))
  phi = torch.asin((Y[..., 0] / rs).clamp(-1, 1))
  theta = torch.atan2(Y[..., 1], Y[..., 2])
  u = (math.pi / 2 - phi) * W / math.pi - 0.5
  v = (math.pi - theta) * H / (2.0 * math.pi) - 0.5
  valid = ok & (u >= 0) & (u <= W - 1)
  return u, v, valid


def slopes(depth, pose):
  """The closed form of the issue: (du/dD, dv/dD) float64, for comparison with autograd."""
  F, H, W = depth.shape
  P = torch.as_tensor(np.asarray(pose, dtype=np.float64).reshape(3, 4))
  m = directions(H, W) @ P[:, :3].T
  Y = depth.double().unsqueeze(-1) * m + P[:, 3]
  r2 = (Y * Y).sum(-1)
  s2 = Y[..., 1] ** 2 + Y[..., 2] ** 2
  dphi = (m[..., 0] * r2 - Y[..., 0] * (Y * m).sum(-1)) / (r2 * s2.sqrt())
  dtheta = (m[..., 1] * Y[..., 2] - m[..., 2] * Y[..., 1]) / s2
  return -(W / math.pi) * dphi, -(H / (2 * math.pi)) * dtheta


def warp(img, depth, pose):
  """img (F, 3, H, W) de-normalised in the working dtype, depth (F, H, W) in the same -> (Ih (F, 3, H, W), valid, u, v)."""
  F, _, H, W = img.shape
  dt = img.dtype
  u, v, valid = project(depth, pose)
  us, vs = torch.where(valid, u, torch.zeros_like(u)), torch.where(valid, v, torch.zeros_like(v))
  x0 = us.detach().floor().clamp(max=W - 2)
  y0 = vs.detach().floor()
  t = (us - x0).to(dt).unsqueeze(1)
  q = (vs - y0).to(dt).unsqueeze(1)
  x0 = x0.long()
  ya, yb = torch.remainder(y0.long(), H), torch.remainder(y0.long() + 1, H)
  flat = img.reshape(F, 3, H * W)

  def at(y, x):
    return flat.gather(2, (y * W + x).unsqueeze(1).expand(F, 3, H, W).reshape(F, 3, H * W)).reshape(F, 3, H, W)

  top = (1 - t) * at(ya, x0) + t * at(ya, x0 + 1)
  bot = (1 - t) * at(yb, x0) + t * at(yb, x0 + 1)
  Ih = (1 - q) * top + q * bot
  return torch.where(valid.unsqueeze(1), Ih, torch.zeros_like(Ih)), valid, u, v


pe_map = R.pe_map  # (L, Ih, valid, alpha) -> (pe (F, H, W - 2), wvalid (F, H, W - 2)): the window term of tests/photometric_ref.py


def smoothness(L, depth, beta):
  good = torch.isfinite(depth) & (depth > 0)
  ld = torch.log(torch.where(good, depth, torch.ones_like(depth)))
  ex = torch.exp(-beta * (L[..., 1:] - L[..., :-1]).abs().mean(1))
  ey = torch.exp(-beta * (torch.roll(L, -1, -2) - L).abs().mean(1))
  gx = good[..., 1:] & good[..., :-1]
  gy = torch.roll(good, -1, -2) & good
  sx = torch.where(gx, (ld[..., 1:] - ld[..., :-1]).abs() * ex, torch.zeros_like(ex))
  sy = torch.where(gy, (torch.roll(ld, -1, -2) - ld).abs() * ey, torch.zeros_like(ey))
  return sx.mean() + sy.mean()


def mv_loss(ref, src, depth, poses, alpha=0.85, lam=0.1, beta=1.0, mean=None, std=None):
  """ref (F, 3, H, W), src (F, S, 3, H, W), depth (F, H, W) in the working dtype (float64 or float32), poses (S, 12) ->
  (loss, info): info = {'N': int, 'win': (F, H, W) uint8 (255 also at columns 0 and W - 1), 'photo', 'smooth', 'pe': (S, F, H, W - 2)
  detached with +inf where the window is invalid, 'u', 'v': (S, F, H, W) float64, 'valid': (S, F, H, W)}."""
  dt = depth.dtype
  mean = torch.tensor(IMAGENET['mean'] if mean is None else mean, dtype=dt).view(1, 3, 1, 1)
  std = torch.tensor(IMAGENET['std'] if std is None else std, dtype=dt).view(1, 3, 1, 1)
  L = ref.to(dt) * std + mean
  F, S, _, H, W = src.shape
  best, idx = None, torch.full((F, H, W - 2), NO_WINNER, dtype=torch.long)
  pes, us, vs, valids = [], [], [], []
  for s in range(S):
    Ih, valid, u, v = warp(src[:, s].to(dt) * std + mean, depth, poses[s])
    pe, wvalid = pe_map(L, Ih, valid, alpha)
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
  smooth = smoothness(L, depth, beta)
  loss = photo + lam * smooth if lam != 0 else photo
  win = torch.full((F, H, W), NO_WINNER, dtype=torch.uint8)
  win[..., 1:-1] = idx.to(torch.uint8)
  return loss, {'N': n, 'win': win, 'photo': photo.detach(), 'smooth': smooth.detach(), 'pe': torch.stack(pes), 'u': torch.stack(us),
                'v': torch.stack(vs), 'valid': torch.stack(valids)}


def make_case(F, H, W, S, seed=None):
  """Seeded float32 inputs: ref (F, 3, H, W), src (F, S, 3, H, W) normalised random images (low-passed uniform noise, the sources half
  the reference's), depth (F, H, W) uniform in [1.5, 8]; poses: the first S of Deep360's default sources."""
  seed = SEEDS.get((F, H, W, S), 0) if seed is None else seed
  g = torch.Generator().manual_seed(1000 * seed + 7 * H + W + 31 * S)
  mean = torch.tensor(IMAGENET['mean']).view(1, 3, 1, 1)
  std = torch.tensor(IMAGENET['std']).view(1, 3, 1, 1)
  base = R._lowpass(torch.rand(F, 3, H, W, generator=g, dtype=torch.float64))
  ref = ((base - mean) / std).float()
  srcs = []
  for _ in range(S):
    other = R._lowpass(torch.rand(F, 3, H, W, generator=g, dtype=torch.float64))
    srcs.append(((0.5 * base + 0.5 * other - mean) / std).float())
  depth = (1.5 + 6.5 * torch.rand(F, H, W, generator=g, dtype=torch.float64)).float()
  return ref, torch.stack(srcs, 1), depth, deep360_poses()[:S]


_cache = {}


def reference(case, dtype, **kw):
  """(loss, info, gdepth) of a case in `dtype` on the CPU, computed once per (case, dtype, parameters) and shared."""
  key = (case, dtype, tuple(sorted(kw.items())))
  if key not in _cache:
    ref, src, depth, poses = make_case(*case)
    _cache[key] = evaluate(ref, src, depth, poses, dtype, **kw)
  return _cache[key]


def evaluate(ref, src, depth, poses, dtype, **kw):
  d = depth.detach().clone().to(dtype).requires_grad_(True)
  loss, info = mv_loss(ref, src, d, poses, **kw)
  g = torch.autograd.grad(loss, d, allow_unused=True)[0] if loss.requires_grad else None
  return loss.detach(), info, torch.zeros_like(d) if g is None else g


yardstick, error = R.yardstick, R.error  # DESIGN 24's bound: the float32 restatement's own error against float64


# ------------------------------------------------------------------------------------------------ a scene with a known answer
SPHERE_RADIUS = 4.0


def texture(X):
  """A low-frequency function of the 3-D point, (..., 3) float64 -> (..., 3) colours in (0, 1)."""
  x, y, z = X[..., 0], X[..., 1], X[..., 2]
  return torch.stack([0.5 + 0.4 * torch.sin(0.9 * x + 0.5 * y) * torch.cos(0.7 * z),
                      0.5 + 0.4 * torch.sin(0.8 * y - 0.6 * z + 1.0),
                      0.5 + 0.4 * torch.cos(0.7 * x + 0.9 * z - 0.4 * y)], -1)


def render_sphere(pose, H, W):
  """The panorama with pose [A | o] of the inside of the textured sphere of radius 4 around the common camera, float64, analytic:
  a camera at c = -A^T o looking along A^T n hits |c + r d| = 4 at r = -c.d + sqrt((c.d)^2 - |c|^2 + 16).  -> (3, H, W) normalised."""
  P = torch.as_tensor(np.asarray(pose, dtype=np.float64).reshape(3, 4))
  A, o = P[:, :3], P[:, 3]
  c = -(A.T @ o)
  d = directions(H, W) @ A  # rows: A^T n
  cd = d @ c
  r = -cd + torch.sqrt(cd * cd - c @ c + SPHERE_RADIUS ** 2)
  X = c + r.unsqueeze(-1) * d
  img = texture(X).permute(2, 0, 1)
  mean = torch.tensor(IMAGENET['mean'], dtype=torch.float64).view(3, 1, 1)
  std = torch.tensor(IMAGENET['std'], dtype=torch.float64).view(3, 1, 1)
  return (img - mean) / std


def sphere_scene(H=64, W=32):
  """-> (ref (1, 3, H, W), src (1, 3, 3, H, W), poses (3, 12)) float64: panoramas 0 and 1, 3, 5 of Deep360."""
  rig = CameraRig.deep360()
  poses = rig.panorama_poses().reshape(-1, 12)
  ref = render_sphere(poses[0], H, W).unsqueeze(0)
  src = torch.stack([render_sphere(poses[s], H, W) for s in (1, 3, 5)]).unsqueeze(0)
  return ref, src, poses[[1, 3, 5]]


def sine_rule_depth(d, W, baseline=1.0):
  """The unclipped sine-rule depth of a disparity map d (..., H, W) float64, angles at pixel centres:
  phi_l = pi/2 - (w + 1/2) pi / W, phi_r = phi_l + d pi / W, depth = b cos(phi_r) / sin(phi_r - phi_l)."""
  w = torch.arange(W, dtype=torch.float64)
  phi_l = math.pi / 2 - (w + 0.5) * math.pi / W
  phi_r = phi_l + d * math.pi / W
  return baseline * torch.cos(phi_r) / torch.sin(phi_r - phi_l)
