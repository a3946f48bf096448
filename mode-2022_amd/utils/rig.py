"""A camera rig as data: which stereo pairs a frame holds, and how each pair's depth map is brought into the common view.

The reference hard-wires one rig, the four cameras of Deep360 on a unit square and their six pairs (save_output_disparity_stage.py:
105-160).  A CameraRig says the same thing in a table, so that utils.geometry.disp2depth_frames_gpu, dataloader.gpu_ingest.frames_u8_gpu
and models.ModeMultiView run on a frame with a camera missing, on a square of another side, or on pairs with poses of the user's own.

A frame of a rig with P pairs is its 2P panoramas, pair-major: panorama 2p is the left image of pair p, panorama 2p + 1 the right one.
"""
import math

import numpy as np

MAX_PAIRS = 16  # the header's MODE_MV_MAX_PAIRS (this module imports no binding; tests/test_rig_host.py holds both values to the header)
KINDS = ('identity', 'rotate', 'view')  # their position is MODE_MV_IDENTITY / MODE_MV_ROTATE / MODE_MV_VIEW
_POSE_LEN = {'identity': 0, 'rotate': 3, 'view': 6}
PAIR_RECORD = np.dtype([('kind', '<i4'), ('table', '<i4'), ('baseline', '<f4')])  # the header's mode_mv_pair


def _rotation(pitch, yaw, roll):
  """R = Rx(roll) Rz(yaw) Ry(pitch) of the PairPose docstring, float64."""
  cp, sp, cy, sy, cr, sr = math.cos(pitch), math.sin(pitch), math.cos(yaw), math.sin(yaw), math.cos(roll), math.sin(roll)
  Ry = np.array([[cp, 0, -sp], [0, 1, 0], [sp, 0, cp]])
  Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
  Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
  return Rx @ Rz @ Ry


def _euler(R):
  """The inverse of _rotation: (pitch, yaw, roll) of an orthonormal R = Rx(roll) Rz(yaw) Ry(pitch), yaw in (-pi/2, pi/2), pitch and
  roll in (-pi, pi].  The first row of R is (cos y cos p, -sin y, -cos y sin p) and its second column (-sin y, cos r cos y,
  sin r cos y).  ValueError within 1e-6 of |yaw| = pi/2, where pitch and roll turn about one axis and only their sum is defined."""
  R = np.asarray(R, dtype=np.float64)
  if R.shape != (3, 3):
    raise ValueError('_euler: R must be 3 x 3, got %s' % (R.shape,))
  cy = math.hypot(R[0][0], R[0][2])
  if cy < math.sin(1e-6):
    raise ValueError('_euler: |yaw| is within 1e-6 of pi/2 (R[0][1] = %.17g): pitch and roll are not separate there' % R[0][1])
  yaw = math.atan2(-R[0][1], cy)  # asin(-R[0][1]), from both the sine and the cosine: asin alone loses digits towards the bound
  pitch = math.atan2(-R[0][2], R[0][0])
  roll = math.atan2(R[2][1], R[1][1])
  return pitch, yaw, roll


def view_pose(centre, rotation=None):
  """(3, 4) float64 [A | o] of a camera that stands at `centre` (in the common view's axes) with orientation R = `rotation` (3 x 3,
  orthonormal to 1e-9; None: the common view's own): A = R^T, o = -A centre, so that X_t = A X + o and the camera stands at -A^T o.
  The inverse of CameraRig.camera_centres(); a target view of HF.mv_render / ModeMultiView.render_views."""
  c = np.asarray(centre, dtype=np.float64)
  if c.shape != (3,) or not np.isfinite(c).all():
    raise ValueError('view_pose: centre must be 3 finite numbers, got %r' % (centre,))
  R = np.eye(3) if rotation is None else np.asarray(rotation, dtype=np.float64)
  if R.shape != (3, 3) or not np.isfinite(R).all() or np.abs(R @ R.T - np.eye(3)).max() > 1e-9:
    raise ValueError('view_pose: rotation must be a 3 x 3 matrix, orthonormal to 1e-9, got %r' % (rotation,))
  A = R.T
  return np.concatenate([A, -(A @ c)[:, None]], 1)


class PairPose(object):
  """One stereo pair of a rig: PairPose(name, baseline, kind, pose=()).

  baseline  the distance between the pair's two cameras, in the unit the depth comes out in (> 0; kept as float32, which is what the
            sine rule  depth = baseline sin(pi/2 - phi_r) / sin(phi_r - phi_l)  computes with).  `exact` keeps the number as it was
            given, in double, for CameraRig.panorama_poses alone.
  kind     how the pair's depth map, which lives in the Cassini frame of the pair's LEFT camera, gets into the common view:
    'identity'  it is there already.  pose = ().
    'rotate'    the left camera stands where the common view's camera stands, turned: the map is resampled as the reference's
                rotateCassini(map, pitch, yaw, roll) resamples it.  pose = (pitch, yaw, roll), radians.
    'view'      the left camera stands elsewhere: every pixel is lifted to its 3-D point, moved and z-buffered into the common view as
                the reference's depthViewTransWithConf(view, conf, y0, z0, x0, pitch, yaw, roll) does.
                pose = (y0, z0, x0, pitch, yaw, roll) -- the translation first, in that (y, z, x) order, then the angles.

  Conventions (the reference's utils/geometry.py:48-156).  A Cassini image of height H and width W has the longitude theta along its
  rows, from +pi (top) to -pi, and the latitude phi along its columns, from +pi/2 (left) to -pi/2.  The pixel (theta, phi) looks along
      x = sin(phi),   y = cos(phi) sin(theta),   z = cos(phi) cos(theta):
  x is the pair's baseline axis (towards the image's left edge), z points at the image's centre row, y at the row a quarter above it.
  The angles make the matrix
      R = Rx(roll) Rz(yaw) Ry(pitch),
      Ry = [[cos p, 0, -sin p], [0, 1, 0], [sin p, 0, cos p]],  Rz = [[cos y, -sin y, 0], [sin y, cos y, 0], [0, 0, 1]],
      Rx = [[1, 0, 0], [0, cos r, -sin r], [0, sin r, cos r]].
  'rotate': the output pixel looking along X2 takes the input's value in the direction X1 = R^-1 X2 (bilinear, border-clamped), i.e.
  R turns the left camera's axes into the common view's.  'view': a point X1 = depth * direction in the left camera's frame becomes
  X2 = R (X1 - t) with t = (x0, y0, z0): t is where the common view's camera stands, in the LEFT camera's axes and in the baseline's
  unit; R is as above.  The nearest point wins a target pixel; its confidence travels with it.
  In Deep360, pair 13 is 'rotate' by a pitch of pi/2 and pair 24 is 'view' from (y0, z0, x0) = (0, -1, 0) with a pitch of pi/2."""

  __slots__ = ('name', 'baseline', 'kind', 'pose', 'exact')

  def __init__(self, name, baseline, kind, pose=()):
    name = str(name)
    if kind not in KINDS:
      raise ValueError("PairPose %r: kind must be one of %s, not %r" % (name, ', '.join(repr(k) for k in KINDS), kind))
    try:
      pose = tuple(float(v) for v in pose)
      b = float(np.float32(baseline))
      exact = float(baseline)
    except (TypeError, ValueError):
      raise ValueError('PairPose %r: baseline and pose must be numbers, got %r and %r' % (name, baseline, pose))
    if not (math.isfinite(b) and b > 0):
      raise ValueError('PairPose %r: baseline must be finite and > 0 in float32, got %r' % (name, baseline))
    if len(pose) != _POSE_LEN[kind]:
      raise ValueError('PairPose %r: a %r pose has %d numbers, got %d' % (name, kind, _POSE_LEN[kind], len(pose)))
    if not all(math.isfinite(v) for v in pose):
      raise ValueError('PairPose %r: pose %r is not finite' % (name, pose))
    object.__setattr__(self, 'name', name)
    object.__setattr__(self, 'baseline', b)
    # The baseline as it was given, before the rounding to float32: what CameraRig.panorama_poses places the right camera with, so
    # that a camera which belongs to several pairs stands at one place (float32(sqrt 2) is 1.7e-8 short of a unit square's diagonal).
    # It is no part of equality, hash or repr, which speak of what the hand-off computes with.
    object.__setattr__(self, 'exact', exact if math.isfinite(exact) and float(np.float32(exact)) == b else b)
    object.__setattr__(self, 'kind', kind)
    object.__setattr__(self, 'pose', pose)

  def __setattr__(self, key, value):
    raise AttributeError('PairPose is immutable')

  def __reduce__(self):  # (copy and pickle rebuild through the constructor: the default protocol restores slots with setattr)
    return (PairPose, (self.name, self.exact, self.kind, self.pose))

  def _key(self):
    return (self.name, self.baseline, self.kind, self.pose)

  def __eq__(self, other):
    return isinstance(other, PairPose) and self._key() == other._key()

  def __ne__(self, other):
    return not self == other

  def __hash__(self):
    return hash(self._key())

  def __repr__(self):
    return 'PairPose(%r, %r, %r, %r)' % self._key()


class CameraRig(object):
  """CameraRig(pairs, rgb, name=None): an ordered sequence of 1 to 16 PairPose entries with distinct names, and `rgb`, the distinct
  panorama indices in [0, 2P), at least one, of the images the fusion network sees.  Immutable and hashable; two rigs are equal when their pairs and
  their rgb are (the name is a label)."""

  __slots__ = ('pairs', 'rgb', 'name')

  def __init__(self, pairs, rgb, name=None):
    pairs = tuple(pairs)
    if not 1 <= len(pairs) <= MAX_PAIRS:
      raise ValueError('CameraRig: %d pairs, not 1 to %d' % (len(pairs), MAX_PAIRS))
    seen = set()
    for k, p in enumerate(pairs):
      if not isinstance(p, PairPose):
        raise ValueError('CameraRig: pair %d is %r, not a PairPose' % (k, type(p)))
      if p.name in seen:
        raise ValueError('CameraRig: pair name %r appears twice' % (p.name,))
      seen.add(p.name)
    try:
      rgb = tuple(int(k) for k in rgb)
    except (TypeError, ValueError):
      raise ValueError('CameraRig: rgb must be a sequence of panorama indices, got %r' % (rgb,))
    for k in rgb:
      if not 0 <= k < 2 * len(pairs):
        raise ValueError('CameraRig: rgb panorama %d is outside [0, %d); panorama 2p / 2p + 1 is the left / right image of pair p (%s)' %
                         (k, 2 * len(pairs), ', '.join(p.name for p in pairs)))
    if len(set(rgb)) != len(rgb):
      raise ValueError('CameraRig: rgb %r names a panorama twice' % (rgb,))
    if not rgb:
      raise ValueError('CameraRig: rgb is empty; the fusion network takes the colour of at least one panorama (ModeFusion has an RGB '
                       'branch, and a convolution over zero planes is none)')
    object.__setattr__(self, 'pairs', pairs)
    object.__setattr__(self, 'rgb', rgb)
    object.__setattr__(self, 'name', name)

  def __setattr__(self, key, value):
    raise AttributeError('CameraRig is immutable')

  def __reduce__(self):  # (as PairPose: a module that holds a rig can be deep-copied, saved whole and sent to loader workers)
    return (CameraRig, (self.pairs, self.rgb, self.name))

  def __eq__(self, other):
    return isinstance(other, CameraRig) and self.pairs == other.pairs and self.rgb == other.rgb

  def __ne__(self, other):
    return not self == other

  def __hash__(self):
    return hash((self.pairs, self.rgb))

  def __len__(self):
    return len(self.pairs)

  def __repr__(self):
    return 'CameraRig(%r, rgb=%r, name=%r)' % (self.pairs, self.rgb, self.name)

  @property
  def names(self):
    return tuple(p.name for p in self.pairs)

  def of_kind(self, kind):
    """The pairs of one kind, in pair order: the order of the rotation grids / the view transforms."""
    return tuple(p for p in self.pairs if p.kind == kind)

  def records(self):
    """(mode_mv_pair records (P,), R, V): kind code, table index -- the pair's ordinal among the pairs of its kind -- and baseline."""
    rec = np.zeros(len(self.pairs), dtype=PAIR_RECORD)
    count = {k: 0 for k in KINDS}
    for i, p in enumerate(self.pairs):
      rec[i] = (KINDS.index(p.kind), count[p.kind], p.baseline)
      count[p.kind] += 1
    return rec, count['rotate'], count['view']

  # ------------------------------------------------------------------------------------------------ panorama poses
  def panorama_poses(self):
    """(2P, 3, 4) float64 [A | o]: a point X in the common view's axes has the coordinates X_s = A_s X + o_s in the Cassini frame of
    panorama s.  From the conventions of PairPose: the left image of an 'identity' pair has A = I, o = 0; of a 'rotate' pair A = R^T,
    o = 0; of a 'view' pair (X2 = R (X1 - t)) A = R^T, o = t.  The right camera of a pair stands at (-b, 0, 0) in the left camera's
    axes with the same orientation -- the sine rule r = b cos(phi_r) / sin(phi_r - phi_l) is tan(phi_r) = (b + r sin(phi_l)) /
    (r cos(phi_l)) -- so the right image has the left's A and the left's o + (b, 0, 0).  The camera of panorama s stands at -A^T o."""
    out = np.zeros((2 * len(self.pairs), 3, 4))
    for k, p in enumerate(self.pairs):
      A, o = np.eye(3), np.zeros(3)
      if p.kind == 'rotate':
        A = _rotation(*p.pose).T
      elif p.kind == 'view':
        y0, z0, x0 = p.pose[:3]
        A, o = _rotation(*p.pose[3:]).T, np.array([x0, y0, z0])
      out[2 * k, :, :3] = out[2 * k + 1, :, :3] = A
      out[2 * k, :, 3] = o
      out[2 * k + 1, :, 3] = o + np.array([p.exact, 0.0, 0.0])
    return out

  def camera_centres(self):
    """(2P, 3) float64: where the camera of every panorama stands, in the common view's axes."""
    poses = self.panorama_poses()
    return -np.einsum('sji,sj->si', poses[:, :, :3], poses[:, :, 3])

  def reference_panorama(self):
    """The first panorama that IS the common view (A = I, o = 0): the image the fused depth map is a depth map of.  ValueError if the
    rig has none: the common view then has no image."""
    for s, pose in enumerate(self.panorama_poses()):
      if np.abs(pose[:, :3] - np.eye(3)).max() <= 1e-12 and np.abs(pose[:, 3]).max() <= 1e-12:
        return s
    raise ValueError('CameraRig.reference_panorama: no panorama of %s is taken from the common view (A = I, o = 0; the left image of an '
                     "'identity' pair is): the common view has no image" % (', '.join(self.names),))

  def default_sources(self):
    """For every distinct camera centre other than the common view's own, the first panorama taken from it, in index order.  A
    panorama at the common view's centre sees every point along the ray of the pixel it is compared with, whatever the depth: it
    carries no depth signal and is never a default source."""
    centres = self.camera_centres()
    scale = max(1.0, float(np.abs(centres).max()))
    seen, out = [np.zeros(3)], []
    for s, c in enumerate(centres):
      if all(np.abs(c - q).max() > 1e-9 * scale for q in seen):
        seen.append(c)
        out.append(s)
    return tuple(out)

  @property
  def deep360_layout(self):
    """Whether a frame has Deep360's layout: six pairs, the fusion RGB at panoramas 0, 1, 10, 11."""
    from dataloader.list_file import _FUSION_RGB
    return len(self.pairs) == 6 and self.rgb == tuple(_FUSION_RGB)

  # ------------------------------------------------------------------------------------------------ constructors
  @classmethod
  def deep360(cls):
    """The rig of Deep360: four cameras on a unit square, pairs 12, 13, 14, 23, 24, 34 in camera 1's frame, from the tables of
    utils.geometry (_baselines('Deep360'), _ROT_PITCH, _VIEW_POSES); the fusion RGB is both images of pair 12 and of pair 34."""
    from . import geometry  # (geometry loads torch and the native package's Python side; the classes above need neither)
    baselines = np.array([1.0, 1.0, math.sqrt(2), math.sqrt(2), 1.0, 1.0])  # PairPose rounds them to float32 and keeps them as given
    assert np.array_equal(baselines.astype(np.float32), geometry._baselines('Deep360'))
    return cls._square(baselines, 1.0, 'Deep360')

  @classmethod
  def square(cls, side, name=None):
    """Deep360's topology on a square of another side: baselines float32(side * (1, 1, sqrt 2, sqrt 2, 1, 1)) and translations side *
    the unit ones, both products formed in double; the rotations are those of Deep360.  square(1.0) == deep360().
    square(0.6 * sqrt(2)) is the self-consistent counterpart of dbname='other': that setting takes the reference's `else` baselines
    (0.6 sqrt 2 and 1.2) but keeps the UNIT square's translations of pairs 23, 24 and 34, as the reference does."""
    side = float(side)
    if not (math.isfinite(side) and side > 0):
      raise ValueError('CameraRig.square: side must be finite and > 0, got %r' % (side,))
    # the unit square's side and diagonal per pair, in double: what utils.geometry._baselines('Deep360') rounds to float32
    unit = np.array([1.0, 1.0, math.sqrt(2), math.sqrt(2), 1.0, 1.0])
    return cls._square(side * unit, side, name if name is not None else 'square(%r)' % side)

  @classmethod
  def _square(cls, baselines, side, name):
    from dataloader.list_file import _FUSION_RGB  # where the fusion lists take the RGB of a Deep360 frame from
    from . import geometry
    pairs = []
    for k, n in enumerate(geometry.PAIRS):
      baseline = baselines[k]
      if n in geometry._ROT_PITCH:
        pairs.append(PairPose(n, baseline, 'rotate', (geometry._ROT_PITCH[n], 0, 0)))
      elif n in geometry._VIEW_POSES:
        pose = geometry._VIEW_POSES[n]
        pairs.append(PairPose(n, baseline, 'view', tuple(side * float(v) for v in pose[:3]) + tuple(pose[3:])))
      else:
        pairs.append(PairPose(n, baseline, 'identity'))
    return cls(pairs, _FUSION_RGB, name=name)

  def subset(self, names, rgb=None):
    """The named pairs, in the order given (which need not be this rig's).  rgb=None keeps those of this rig's RGB panoramas whose
    pair is among them, renumbered, in this rig's order; ValueError if none is."""
    names = tuple(str(n) for n in names)
    have = self.names
    for n in names:
      if n not in have:
        raise ValueError('CameraRig.subset: no pair %r among %s' % (n, ', '.join(have)))
    if rgb is None:
      rgb = tuple(2 * names.index(have[k // 2]) + k % 2 for k in self.rgb if have[k // 2] in names)
      if not rgb:
        raise ValueError('CameraRig.subset: none of the RGB panoramas %r (pairs %s) belongs to the pairs %s; pass rgb=' %
                         (self.rgb, ', '.join(sorted({have[k // 2] for k in self.rgb})), ', '.join(names)))
    return CameraRig([self.pairs[have.index(n)] for n in names], rgb, name='%s[%s]' % (self.name, ','.join(names)))
