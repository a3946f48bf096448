"""The multi-view reprojection loss of DESIGN 25 restated with the POSES as a tensor (HF.mv_photometric_loss with a pose
tensor, csrc/mv_pose_grad.hip): tests/mvphoto_ref.py's loss with its own project, warp and mv_loss, so that autograd reaches
[A | o]; the closed form of include/mode_hip_mvpose.h; generic (perturbed) poses and the seeded cases the tests share.

With the poses detached every operation here is mvphoto_ref's, in the same order: loss, win and N are torch.equal
(tests/test_mvpose_host.py).  pe_map, smoothness, make_case, the sphere scene, yardstick and error are mvphoto_ref's own.

The geometry (u, v) is float64 in both restatements, as in the kernel; the float32 one rounds at t and q, and autograd rounds the
slopes where they meet the float32 bilinear."""
import math

import numpy as np
import torch

import mvphoto_ref as M

CASES = M.CASES
# One pose seed per case, searched (0, 1, ...) for the first at which the conditions of tests/test_mvpose_host.py hold.
SEEDS = {CASES[0]: 1, CASES[1]: 0, CASES[2]: 1, CASES[3]: 2}
NO_WINNER = M.NO_WINNER
pe_map, smoothness, yardstick, error = M.pe_map, M.smoothness, M.yardstick, M.error


def skew(w):
  z = torch.zeros_like(w[..., 0])
  return torch.stack([torch.stack([z, -w[..., 2], w[..., 1]], -1), torch.stack([w[..., 2], z, -w[..., 0]], -1),
                      torch.stack([-w[..., 1], w[..., 0], z], -1)], -2)


def twisted(poses, twist):
  """poses (S, 12) float64 tensor, twist (S, 6) = (omega, tau) -> (S, 12): A' = Exp(omega) A, o' = Exp(omega) o + tau."""
  P = poses.reshape(-1, 3, 4)
  E = torch.linalg.matrix_exp(skew(twist[:, :3]))
  return torch.cat([E @ P[:, :, :3], E @ P[:, :, 3:] + twist[:, 3:].unsqueeze(-1)], -1).reshape(-1, 12)


def perturbed_poses(S, seed, sources=None):
  """(S, 12) float64 numpy: Deep360's sources (the first S default ones, or those named), each left-multiplied by Exp of a rotation
  vector uniform in +-0.005 per component and shifted by a vector uniform in +-0.01: generic poses, no u or v on an integer."""
  base = M.deep360_poses(sources)[:S].reshape(S, 3, 4)
  g = torch.Generator().manual_seed(4321 + seed)
  rot = (torch.rand(S, 3, generator=g, dtype=torch.float64) * 2 - 1) * 0.005
  shift = (torch.rand(S, 3, generator=g, dtype=torch.float64) * 2 - 1) * 0.01
  E = torch.linalg.matrix_exp(skew(rot)).numpy()
  out = base.copy()
  out[:, :, :3] = E @ base[:, :, :3]
  out[:, :, 3] += shift.numpy()
  return np.ascontiguousarray(out.reshape(S, 12))


def make_case(F, H, W, S):
  """mvphoto_ref.make_case's images and depth with this module's perturbed poses -> (ref, src, depth, poses (S, 12) numpy)."""
  ref, src, depth, _ = M.make_case(F, H, W, S)
  return ref, src, depth, perturbed_poses(S, SEEDS[(F, H, W, S)])


def project(depth, pose):
  """depth (F, H, W) any float dtype, pose (12,) float64 TENSOR -> (u, v (F, H, W) float64 with autograd through depth and pose, valid,
  Y (F, H, W, 3)): mvphoto_ref.project, operation for operation."""
  F, H, W = depth.shape
  P = pose.reshape(3, 4)
  D = depth.double()
  good = torch.isfinite(D) & (D > 0)
  Ds = torch.where(good, D, torch.ones_like(D))
  m = M.directions(H, W) @ P[:, :3].T  # (H, W, 3)
  Y = Ds.unsqueeze(-1) * m + P[:, 3]
  rho = Y.norm(dim=-1)
  ok = good & (rho > 0)
  rs = torch.where(ok, rho, torch.ones_like(rho))
  phi = torch.asin((Y[..., 0] / rs).clamp(-1, 1))
  theta = torch.atan2(Y[..., 1], Y[..., 2])
  u = (math.pi / 2 - phi) * W / math.pi - 0.5
  v = (math.pi - theta) * H / (2.0 * math.pi) - 0.5
  valid = ok & (u >= 0) & (u <= W - 1)
  return u, v, valid, Y


def warp(img, depth, pose):
  """img (F, 3, H, W) de-normalised in the working dtype, depth (F, H, W) in the same, pose (12,) tensor ->
  (Ih (F, 3, H, W), valid, u, v, Iu, Iv, Y): Iu, Iv the bilinear's two partial slopes (detached), Y the point in the source's frame."""
  F, _, H, W = img.shape
  dt = img.dtype
  u, v, valid, Y = project(depth, pose)
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

  r00, r01, r10, r11 = at(ya, x0), at(ya, x0 + 1), at(yb, x0), at(yb, x0 + 1)
  top = (1 - t) * r00 + t * r01
  bot = (1 - t) * r10 + t * r11
  Ih = (1 - q) * top + q * bot
  zero = torch.zeros_like(Ih)
  with torch.no_grad():
    Iu = torch.where(valid.unsqueeze(1), (1 - q) * (r01 - r00) + q * (r11 - r10), zero)
    Iv = torch.where(valid.unsqueeze(1), bot - top, zero)
  return torch.where(valid.unsqueeze(1), Ih, zero), valid, u, v, Iu, Iv, Y


def _minimum(L, Ihs, valids, alpha):
  """The per-window minimum of mvphoto_ref.mv_loss over the warped sources -> (best, idx, pes)."""
  F, _, H, W = L.shape
  best, idx = None, torch.full((F, H, W - 2), NO_WINNER, dtype=torch.long)
  pes = []
  for s, (Ih, valid) in enumerate(zip(Ihs, valids)):
    pe, wvalid = pe_map(L, Ih, valid, alpha)
    better = wvalid & ((idx == NO_WINNER) | (pe.detach() < (best.detach() if best is not None else pe.detach())))
    best = torch.where(better, pe, best if best is not None else torch.zeros_like(pe))
    idx = torch.where(better, torch.full_like(idx, s), idx)
    pes.append(torch.where(wvalid, pe.detach(), torch.full_like(pe, float('inf')).detach()))
  return best, idx, pes


def mv_loss(ref, src, depth, poses, alpha=0.85, lam=0.1, beta=1.0, mean=None, std=None):
  """mvphoto_ref.mv_loss with poses (S, 12) a float64 TENSOR (autograd into it): -> (loss, info); info as there."""
  dt = depth.dtype
  mean = torch.tensor(M.IMAGENET['mean'] if mean is None else mean, dtype=dt).view(1, 3, 1, 1)
  std = torch.tensor(M.IMAGENET['std'] if std is None else std, dtype=dt).view(1, 3, 1, 1)
  L = ref.to(dt) * std + mean
  F, S, _, H, W = src.shape
  warped = [warp(src[:, s].to(dt) * std + mean, depth, poses[s]) for s in range(S)]
  best, idx, pes = _minimum(L, [w[0] for w in warped], [w[1] for w in warped], alpha)
  has = idx != NO_WINNER
  n = int(has.sum())
  photo = torch.where(has, best, torch.zeros_like(best)).sum() / max(n, 1)
  smooth = smoothness(L, depth, beta)
  loss = photo + lam * smooth if lam != 0 else photo
  win = torch.full((F, H, W), NO_WINNER, dtype=torch.uint8)
  win[..., 1:-1] = idx.to(torch.uint8)
  return loss, {'N': n, 'win': win, 'photo': photo.detach(), 'smooth': smooth.detach(), 'pe': torch.stack(pes),
                'u': torch.stack([w[2].detach() for w in warped]), 'v': torch.stack([w[3].detach() for w in warped]),
                'valid': torch.stack([w[1] for w in warped])}


def closed_form(ref, src, depth, poses, alpha=0.85, mean=None, std=None):
  """The definition of include/mode_hip_mvpose.h in float64, without autograd through the geometry: a_c from autograd through the
  windows alone (Ih_s a leaf), G_u, G_v, the two Jacobians in closed form, and the sum over the pixels -> gposes (S, 12) for gloss = 1."""
  dt = torch.float64
  poses = torch.as_tensor(poses, dtype=dt).reshape(-1, 12)
  depth = depth.to(dt)
  mean = torch.tensor(M.IMAGENET['mean'] if mean is None else mean, dtype=dt).view(1, 3, 1, 1)
  std = torch.tensor(M.IMAGENET['std'] if std is None else std, dtype=dt).view(1, 3, 1, 1)
  L = ref.to(dt) * std + mean
  F, S, _, H, W = src.shape
  warped = [warp(src[:, s].to(dt) * std + mean, depth, poses[s]) for s in range(S)]
  leaves = [w[0].detach().requires_grad_(True) for w in warped]
  best, idx, _ = _minimum(L, leaves, [w[1] for w in warped], alpha)
  has = idx != NO_WINNER
  n = int(has.sum())
  total = torch.where(has, best, torch.zeros_like(best)).sum()
  a = torch.autograd.grad(total, leaves, allow_unused=True) if total.requires_grad else [None] * S
  X = depth.unsqueeze(-1) * M.directions(H, W)  # D n
  X4 = torch.cat([X, torch.ones_like(X[..., :1])], -1)
  out = torch.zeros(S, 12, dtype=dt)
  for s in range(S):
    if a[s] is None:
      continue
    _, valid, _, _, Iu, Iv, Y = warped[s]
    Gu, Gv = (a[s] * Iu).sum(1), (a[s] * Iv).sum(1)
    Yx, Yy, Yz = Y[..., 0], Y[..., 1], Y[..., 2]
    s2 = Yy * Yy + Yz * Yz
    r2 = Yx * Yx + s2
    ex = torch.stack([torch.ones_like(Yx), torch.zeros_like(Yx), torch.zeros_like(Yx)], -1)
    gu = -(W / math.pi) * (ex * r2.unsqueeze(-1) - Yx.unsqueeze(-1) * Y) / (r2 * s2.sqrt()).unsqueeze(-1)
    gv = -(H / (2 * math.pi)) * torch.stack([torch.zeros_like(Yx), Yz, -Yy], -1) / s2.unsqueeze(-1)
    gY = Gu.unsqueeze(-1) * gu + Gv.unsqueeze(-1) * gv
    gY = torch.where(valid.unsqueeze(-1), gY, torch.zeros_like(gY))
    out[s] = torch.einsum('fhwa,fhwb->ab', gY, torch.where(valid.unsqueeze(-1), X4, torch.zeros_like(X4))).reshape(12) / max(n, 1)
  return out


def evaluate(ref, src, depth, poses, dtype, **kw):
  """-> (loss, info, gposes (S, 12) float64) of the restatement in `dtype` (the geometry and the poses are float64 in both)."""
  P = torch.as_tensor(np.asarray(poses, dtype=np.float64)).reshape(-1, 12).clone().requires_grad_(True)
  loss, info = mv_loss(ref, src, depth.detach().to(dtype), P, **kw)
  g = torch.autograd.grad(loss, P, allow_unused=True)[0] if loss.requires_grad else None
  return loss.detach(), info, torch.zeros_like(P) if g is None else g


def known_answer(source, loss_of, steps=100, seed=5, H=64, W=32):
  """The run with a known answer: the analytic sphere of mvphoto_ref at H x W seen from Deep360's true poses, D = 4 (the truth),
  lam = 0; a RigRefinement started from a seeded twist (rotation uniform in +-0.02, translation in +-0.05, under the mask), Adam with
  lr = 2e-3, `steps` steps on panorama `source` alone.  loss_of(ref (1, 3, H, W), src (1, 1, 3, H, W), depth (1, H, W), poses (1, 12)
  tensor) -> loss.  -> ((rotation error, translation error) at the start, the same at the end): |A' A^T - I|_F / sqrt 2 and |o' - o|."""
  from utils.rig import CameraRig
  from utils.rig_refine import RigRefinement
  rig = CameraRig.deep360()
  refine = RigRefinement(rig)
  true = torch.from_numpy(rig.panorama_poses())
  g = torch.Generator().manual_seed(seed)
  P = len(rig.pairs)
  start = torch.cat([(torch.rand(P, 3, generator=g, dtype=torch.float64) * 2 - 1) * 0.02,
                     (torch.rand(P, 3, generator=g, dtype=torch.float64) * 2 - 1) * 0.05], 1) * refine.mask
  with torch.no_grad():
    refine.twist.copy_(start)
  ref = M.render_sphere(true[0].reshape(12), H, W).unsqueeze(0)
  src = M.render_sphere(true[source].reshape(12), H, W).reshape(1, 1, 3, H, W)
  depth = torch.full((1, H, W), M.SPHERE_RADIUS, dtype=torch.float64)

  def errors():
    with torch.no_grad():
      p = refine()[source]
    A, A0 = p[:, :3], true[source, :, :3]
    return float((A @ A0.T - torch.eye(3, dtype=torch.float64)).norm()) / math.sqrt(2), float((p[:, 3] - true[source, :, 3]).norm())

  before = errors()
  opt = torch.optim.Adam(refine.parameters(), lr=2e-3)
  for _ in range(steps):
    opt.zero_grad()
    loss = loss_of(ref, src, depth, refine()[source].reshape(1, 12))
    loss.backward()
    opt.step()
  return before, errors()


_cache = {}


def reference(case, dtype, **kw):
  """(loss, info, gposes) of a case in `dtype` on the CPU, computed once per (case, dtype, parameters) and shared."""
  key = (case, dtype, tuple(sorted(kw.items())))
  if key not in _cache:
    _cache[key] = evaluate(*make_case(*case), dtype, **kw)
  return _cache[key]


def conditions(case, poses=None):
  """What the exact comparisons rest on, measured on the restatement -> dict(near: the smallest distance of a valid u or v from an
  integer, err: the float32 restatement's largest pe error, gap: the smallest gap between the best and the second-best pe_s,
  same: float32 and float64 agree on every win and validity, frac: the share of windows with a winner)."""
  ref, src, depth, p = make_case(*case)
  return conditions_of(ref, src, depth, p if poses is None else poses)


def conditions_of(ref, src, depth, poses, **kw):
  """conditions for any inputs."""
  F, S, _, H, W = src.shape
  _, i64, _ = evaluate(ref, src, depth, poses, torch.float64, **kw)
  _, i32, _ = evaluate(ref, src, depth, poses, torch.float32, **kw)
  ok = i64['valid']
  near = min(float((x - x.round()).abs()[ok].min()) for x in (i64['u'], i64['v']))
  fin = torch.isfinite(i64['pe'])
  same = torch.equal(fin, torch.isfinite(i32['pe'])) and torch.equal(i32['valid'], i64['valid']) and torch.equal(i32['win'], i64['win'])
  err = float((i32['pe'].double() - i64['pe'])[fin & torch.isfinite(i32['pe'])].abs().max())
  gap = float('inf')
  if S > 1:
    srt = torch.sort(i64['pe'], 0).values
    both = torch.isfinite(srt[1])
    gap = float((srt[1] - srt[0])[both].min()) if bool(both.any()) else gap
  return {'near': near, 'err': err, 'gap': gap, 'same': same, 'frac': i64['N'] / float(F * H * (W - 2))}
