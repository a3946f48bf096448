"""Self-calibration of a rig: the extrinsics of a CameraRig as parameters that the reprojection loss can move, and the way
back into a CameraRig so that the refined extrinsics also reach the hand-off.

    refine = RigRefinement(rig)                                          # float64, on the host
    opt = torch.optim.Adam(refine.parameters(), lr=2e-3)
    loss, _ = net.fusion_selfsup_loss(frames, sources=(7,), poses=refine())   # HF.mv_photometric_loss carries the gradient to the poses
    loss.backward(); opt.step()
    net.rig = refine.refined_rig()

utils/rig.py stays free of torch; this module is where the two meet.

What the loss can and cannot tell (include/mode_hip_mvpose.h): a source that wins no window gets no gradient, so a miscalibrated source
that loses against a well-calibrated one nearly everywhere converges slowly or not at all -- calibrate a source at a time (sources=),
or only sources that are comparably off.  The baselines are not refined: they fix the scale."""
import torch
from torch import nn

from .rig import CameraRig, PairPose, _euler


def _skew(w):
  """(..., 3) -> (..., 3, 3): the matrix of w x ."""
  z = torch.zeros_like(w[..., 0])
  return torch.stack([torch.stack([z, -w[..., 2], w[..., 1]], -1),
                      torch.stack([w[..., 2], z, -w[..., 0]], -1),
                      torch.stack([-w[..., 1], w[..., 0], z], -1)], -2)


class RigRefinement(nn.Module):
  """RigRefinement(rig, rotation=True, translation=True): one parameter, twist (P, 6) float64 = (omega, tau) per pair, zeros at the
  start.  It is a left perturbation in the pair's own frame, applied to both panoramas of the pair so that the pair stays rectified:
      A' = Exp(omega) A,   o'_left = Exp(omega) o_left + tau,   o'_right = o'_left + (b, 0, 0)       (b = the pair's PairPose.exact)
  Exp is torch.linalg.matrix_exp of the skew matrix: differentiable at 0 and orthonormal to 1e-15.  A fixed 0 / 1 mask freezes what
  must not move: an 'identity' pair has no free parameter (it is the common view), a 'rotate' pair has omega only (o = 0 is what
  makes it 'rotate'), a 'view' pair has both; rotation=False / translation=False clear those columns for every pair.  Masked entries
  of twist have no effect and get an exactly zero gradient.

  forward() -> the (2P, 3, 4) poses in the order of rig.panorama_poses(), with autograd into twist.
  refined_rig() -> a CameraRig with the same pairs, names, kinds, baselines and rgb and the refined poses in PairPose.pose."""

  def __init__(self, rig, rotation=True, translation=True):
    super().__init__()
    if not isinstance(rig, CameraRig):
      raise ValueError('RigRefinement: rig must be a CameraRig, got %r' % (type(rig),))
    self.rig = rig
    base = torch.from_numpy(rig.panorama_poses())
    mask = torch.zeros(len(rig.pairs), 6, dtype=torch.float64)
    for k, p in enumerate(rig.pairs):
      if p.kind in ('rotate', 'view') and rotation:
        mask[k, :3] = 1
      if p.kind == 'view' and translation:
        mask[k, 3:] = 1
    self.register_buffer('left', base[0::2].clone())  # (P, 3, 4): the left panorama of every pair
    self.register_buffer('baseline', torch.tensor([[p.exact, 0.0, 0.0] for p in rig.pairs], dtype=torch.float64))
    self.register_buffer('mask', mask)
    self.twist = nn.Parameter(torch.zeros(len(rig.pairs), 6, dtype=torch.float64))

  def forward(self):
    tw = self.twist * self.mask
    E = torch.linalg.matrix_exp(_skew(tw[:, :3]))  # (P, 3, 3)
    A = E @ self.left[:, :, :3]
    o = (E @ self.left[:, :, 3:])[..., 0] + tw[:, 3:]
    left = torch.cat([A, o.unsqueeze(-1)], -1)
    right = torch.cat([A, (o + self.baseline).unsqueeze(-1)], -1)
    return torch.stack([left, right], 1).reshape(-1, 3, 4)

  def refined_rig(self):
    """The rig with the refined poses written back: R = A'^T = Rx(roll) Rz(yaw) Ry(pitch) through utils.rig._euler (ValueError within
    1e-6 of |yaw| = pi/2) and (y0, z0, x0) from o'_left.  A pair whose free twist entries are all zero keeps its PairPose as it is."""
    with torch.no_grad():
      poses = self.forward()[0::2].numpy()
      moved = (self.twist * self.mask).ne(0).any(1).tolist()
    pairs = []
    for k, p in enumerate(self.rig.pairs):
      if not moved[k]:
        pairs.append(p)
        continue
      angles = _euler(poses[k, :, :3].T)
      o = poses[k, :, 3]
      pose = angles if p.kind == 'rotate' else (float(o[1]), float(o[2]), float(o[0])) + angles
      pairs.append(PairPose(p.name, p.exact, p.kind, pose))
    return CameraRig(pairs, self.rig.rgb, name=self.rig.name)
