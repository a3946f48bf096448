"""Export-stage geometry of the disparity network, MI355X edition.

Drop-in for the functions of the reference's ``utils/geometry.py`` (cassini2Equirec, rotateCassini, depthViewTransWithConf,
erp2rect_cassini) and for ``disp2depth`` of ``save_output_disparity_stage.py:105-160``: same names, arguments and return
conventions (numpy in, numpy out).  The reference builds angle maps with numpy, ships them to the GPU for one
``F.grid_sample`` and back, and runs the z-buffer of the view transform as a sequential numba loop on the CPU.  Here the
angle maps (functions of the image size and the rotation only) are still built with numpy -- they are what defines the
geometry -- but are cached and kept on the device, and everything per pixel runs in libmode_hip.so
(csrc/geometry.hip): ``*_gpu`` variants take and return device tensors so that a pipeline never leaves the GPU.

There is no CPU path: the native library is required (the reference, too, hard-codes ``.cuda()``).
"""
import functools
import math
import threading

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from mode_hip import CONSTANTS, check, lib, ptr, require_f32c, require_gpu, stream_of
from mode_hip import functional as _HF

_DEV = 'cuda'


def _ranges(output_h, output_w):
  """theta over the h axis (longitude, 2 pi) and phi over the w axis (latitude, pi) of a Cassini image, as float64 ranges
  (geometry.py:64-74): np.arange(start, end, -step)."""
  theta = np.arange(np.pi - (np.pi / output_h), -np.pi, -(2 * np.pi / output_h))
  phi = np.arange(0.5 * np.pi - (0.5 * np.pi / output_w), -0.5 * np.pi, -(np.pi / output_w))
  return theta, phi


def _cassini_angle_maps(output_h, output_w):
  """float32 (H, W) maps theta[i], phi[j] exactly as the reference builds them (list of ranges -> float32 array)."""
  theta, phi = _ranges(output_h, output_w)
  theta_map = np.broadcast_to(theta.astype(np.float32)[:, None], (output_h, output_w))
  phi_map = np.broadcast_to(phi.astype(np.float32)[None, :], (output_h, output_w))
  return theta_map, phi_map


def _rotation(pitch, yaw, roll):
  """R = Rx(roll) Rz(yaw) Ry(pitch), geometry.py:49-55."""
  Rx = np.array([[1, 0, 0], [0, np.cos(roll), -np.sin(roll)], [0, np.sin(roll), np.cos(roll)]])
  Rz = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
  Ry = np.array([[np.cos(pitch), 0, -np.sin(pitch)], [0, 1, 0], [np.sin(pitch), 0, np.cos(pitch)]])
  return np.dot(np.dot(Rx, Rz), Ry)


def _unit_dirs(output_h, output_w):
  """(3, H, W) float32: sin(phi), cos(phi) sin(theta), cos(phi) cos(theta) (geometry.py:76-78, 126-128 without the radius)."""
  theta_map, phi_map = _cassini_angle_maps(output_h, output_w)
  return np.stack((np.sin(phi_map), np.cos(phi_map) * np.sin(theta_map), np.cos(phi_map) * np.cos(theta_map))).astype(np.float32)


@functools.lru_cache(maxsize=32)
def _trig_device(output_h, output_w, device):
  """sin phi[W], cos phi[W], sin theta[H], cos theta[H] as numpy's float32 sin / cos of the float32 angle ranges."""
  theta, phi = _ranges(output_h, output_w)
  theta, phi = theta.astype(np.float32), phi.astype(np.float32)
  return torch.from_numpy(np.concatenate((np.sin(phi), np.cos(phi), np.sin(theta), np.cos(theta))).astype(np.float32)).to(device)


def _grid_sample(src, grid):
  """src (N,C,Hs,Ws), grid (1|N,Ho,Wo,2) device tensors -> (N,C,Ho,Wo); bilinear, border padding, align_corners=True."""
  require_gpu(src, grid)
  src, grid = src.contiguous(), grid.contiguous()
  require_f32c(src, grid)
  N, C, Hs, Ws = src.shape
  G, Ho, Wo, two = grid.shape
  if two != 2 or G not in (1, N):
    raise RuntimeError('grid_sample: grid %s does not fit input %s' % (tuple(grid.shape), tuple(src.shape)))
  dst = torch.empty((N, C, Ho, Wo), dtype=src.dtype, device=src.device)
  with torch.cuda.device_of(src):
    check(lib().mode_grid_sample_border(ptr(src), ptr(grid), ptr(dst), N, C, Hs, Ws, Ho, Wo, G, stream_of(src)), 'mode_grid_sample_border')
  return dst


def _to_nchw(img):
  """numpy (H, W) or (H, W, C) -> device (1, C, H, W) float32, as `torch.FloatTensor(img).unsqueeze(0).transpose(1, 3).transpose(2, 3)`."""
  a = np.asarray(img)
  if a.ndim == 2:
    a = a[:, :, None]
  return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)).astype(np.float32)).unsqueeze(0).to(_DEV)


def _from_nchw(sampled, like):
  return sampled[0].permute(1, 2, 0).cpu().numpy().astype(np.asarray(like).dtype)


# ------------------------------------------------------------------------------------------------ rotateCassini
@functools.lru_cache(maxsize=32)
def _rotate_grid(output_h, output_w, pitch, yaw, roll, device):
  R_I = np.linalg.inv(_rotation(pitch, yaw, roll))
  dirs = _unit_dirs(output_h, output_w)
  X_2 = np.expand_dims(np.dstack((dirs[0], dirs[1], dirs[2])), axis=-1)
  X_1 = np.matmul(R_I, X_2)
  theta_1_map = np.arctan2(X_1[:, :, 1, 0], X_1[:, :, 2, 0])
  phi_1_map = np.arcsin(np.clip(X_1[:, :, 0, 0], -1, 1))
  grid = np.stack((np.clip(-phi_1_map / (0.5 * np.pi), -1, 1), np.clip(-theta_1_map / np.pi, -1, 1)), axis=-1).astype(np.float32)
  return torch.from_numpy(grid).unsqueeze(0).to(device)


def rotateCassini_gpu(src, pitch, yaw, roll):
  """src (N, C, H, W) device tensor -> the same views rotated (geometry.py:48-96)."""
  return _grid_sample(src, _rotate_grid(src.shape[2], src.shape[3], float(pitch), float(yaw), float(roll), str(src.device)))


def rotateCassini(cassini_1, pitch, yaw, roll):
  """numpy (H, W, C) -> numpy (H, W, C) of the same dtype."""
  return _from_nchw(rotateCassini_gpu(_to_nchw(cassini_1), pitch, yaw, roll), cassini_1)


# ------------------------------------------------------------------------------------------------ cassini2Equirec
@functools.lru_cache(maxsize=32)
def _c2e_grid(erp_h, erp_w, device):
  theta_erp = np.arange(np.pi - (np.pi / erp_w), -np.pi, -(2 * np.pi / erp_w))
  phi_erp = np.arange(0.5 * np.pi - (0.5 * np.pi / erp_h), -0.5 * np.pi, -(np.pi / erp_h))
  theta_erp_map = np.broadcast_to(theta_erp.astype(np.float32)[None, :], (erp_h, erp_w))
  phi_erp_map = np.broadcast_to(phi_erp.astype(np.float32)[:, None], (erp_h, erp_w))
  theta_cassini_map = np.arctan2(np.tan(phi_erp_map), np.cos(theta_erp_map))
  phi_cassini_map = np.arcsin(np.cos(phi_erp_map) * np.sin(theta_erp_map))
  grid = np.stack((np.clip(-phi_cassini_map / (0.5 * np.pi), -1, 1), np.clip(-theta_cassini_map / np.pi, -1, 1)), axis=-1).astype(np.float32)
  return torch.from_numpy(grid).unsqueeze(0).to(device)


def cassini2Equirec(cassini):
  """geometry.py:7-45: Cassini (H=2h, W=h) image(s) -> equirectangular (h, 2h).  numpy (H,W) / (H,W,C) -> numpy, squeezed;
  a 4D device tensor (N,C,H,W) -> device tensor (N,C,h,2h) squeezed on dim 1, as the reference does."""
  if isinstance(cassini, torch.Tensor) and cassini.dim() == 4:
    src = cassini
    return _grid_sample(src, _c2e_grid(src.shape[-1], src.shape[-2], str(src.device))).squeeze(1)
  a = np.asarray(cassini)
  if a.ndim not in (2, 3):
    raise ValueError('cassini2Equirec: expected a 2D/3D array or a 4D tensor')
  src = _to_nchw(a)
  out = _grid_sample(src, _c2e_grid(src.shape[-1], src.shape[-2], str(src.device)))
  return _from_nchw(out, a).squeeze()


# ------------------------------------------------------------------------------------------------ the rotations of the 3D60 pairs
# rotation vectors of the 3D60 stereo pairs as the reference writes them (dataloader/dataset3D60Loader.py:141, 147, 153): float32
PAIR_VECTORS = {'lr': np.array([0, 0, 0]).astype(np.float32), 'ud': np.array([0, 0, -np.pi / 2]).astype(np.float32),
                'ur': np.array([0, 0, -np.pi / 4]).astype(np.float32)}


def rodrigues(rvec):
  """Rotation vector -> 3x3 matrix by Rodrigues' formula, R = cos(t) I + (1 - cos(t)) r r^T + sin(t) [r]x with t = |rvec|, r = rvec / t,
  evaluated in float64 and returned in the vector's dtype, which is what cv2.Rodrigues does.  (The reference calls cv2.Rodrigues; cv2
  is not a dependency here, so its last bits for a non-zero rotation are not pinned.  The zero vector gives the exact identity.)"""
  v = np.asarray(rvec)
  r = v.astype(np.float64).reshape(3)
  theta = float(np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]))
  if theta < np.finfo(np.float64).eps:
    return np.eye(3, dtype=v.dtype)
  c, s = np.cos(theta), np.sin(theta)
  r = r / theta
  rrt = np.outer(r, r)
  r_x = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
  return (c * np.eye(3) + (1 - c) * rrt + s * r_x).astype(v.dtype)


def pair_rotation(pair):
  """The float32 rotation matrix of a 3D60 stereo pair ('lr', 'ud' or 'ur'), dataset3D60Loader.py:136-153, 175."""
  if pair not in PAIR_VECTORS:
    raise ValueError("3D60 pair %r is not one of 'lr', 'ud', 'ur'" % (pair,))
  return rodrigues(PAIR_VECTORS[pair])


# ------------------------------------------------------------------------------------------------ erp2rect_cassini
_erp2rect_grids = {}  # (bytes of R, its dtype and shape, ca_h, ca_w) -> read-only float32 (ca_h, ca_w, 2); bounded below
_erp2rect_lock = threading.Lock()


def erp2rect_grid(R, ca_h, ca_w):
  """The sample points of erp2rect_cassini (geometry.py:170-193) as a float32 (ca_h, ca_w, 2) array of normalised (x, y): for every
  pixel of the rectified Cassini image the point of the equirectangular source, under rotation R (3x3).  A function of (R, ca_h, ca_w)
  alone, cached (the array is shared and read-only)."""
  R = np.asarray(R)
  key = (R.tobytes(), R.dtype.str, R.shape, int(ca_h), int(ca_w))
  with _erp2rect_lock:
    hit = _erp2rect_grids.get(key)
    if hit is None:
      dirs = _unit_dirs(ca_h, ca_w)
      X = np.expand_dims(np.dstack((dirs[0], dirs[1], dirs[2])), axis=-1)
      X2 = np.matmul(np.linalg.inv(R), X)
      phi_erp_map = np.arcsin(X2[:, :, 1, :])
      theta_erp_map = np.arctan2(X2[:, :, 0, :], X2[:, :, 2, :])
      hit = np.concatenate((np.clip(-theta_erp_map / np.pi, -1, 1), np.clip(-phi_erp_map / (0.5 * np.pi), -1, 1)), axis=-1).astype(np.float32)
      hit.setflags(write=False)
      if len(_erp2rect_grids) >= 32:
        _erp2rect_grids.pop(next(iter(_erp2rect_grids)))
      _erp2rect_grids[key] = hit
    return hit


def erp2rect_cassini(erp, R, ca_h, ca_w, devcice='cuda'):
  """geometry.py:160-198: equirectangular image -> rectified Cassini (ca_h, ca_w) under rotation R (3x3).  The misspelt
  keyword is the reference's."""
  grid = torch.from_numpy(erp2rect_grid(R, ca_h, ca_w).copy()).unsqueeze(0).to(devcice)
  if isinstance(erp, torch.Tensor) and erp.dim() == 4:
    return _grid_sample(erp, grid).squeeze(1)
  a = np.asarray(erp)
  out = _grid_sample(_to_nchw(a).to(devcice), grid)
  return _from_nchw(out, a).squeeze()


# ------------------------------------------------------------------------------------------------ depthViewTransWithConf
def depthViewTransWithConf_gpu(view_1, conf_1, y0, z0, x0, pitch, yaw, roll):
  """view_1, conf_1: (H, W) float32 device tensors -> (view_2, conf_2) device tensors (geometry.py:99-156)."""
  require_gpu(view_1, conf_1)
  view_1, conf_1 = view_1.contiguous(), conf_1.contiguous()
  require_f32c(view_1, conf_1)
  H, W = view_1.shape
  R = np.ascontiguousarray(_rotation(pitch, yaw, roll), dtype=np.float64)
  t = np.array([x0, y0, z0], dtype=np.float64)
  trig = _trig_device(H, W, str(view_1.device))
  view_2, conf_2 = torch.empty_like(view_1), torch.empty_like(view_1)
  ws = torch.empty(lib().mode_depth_view_trans_workspace_bytes(H, W) // 8, dtype=torch.int64, device=view_1.device)
  with torch.cuda.device_of(view_1):
    check(lib().mode_depth_view_trans(ptr(view_1), ptr(conf_1), ptr(trig), R.ctypes.data, t.ctypes.data, ptr(view_2), ptr(conf_2), ptr(ws),
                                      H, W, stream_of(view_1)), 'mode_depth_view_trans')
  return view_2, conf_2


def project_gpu(view_1, y0, z0, x0, pitch, yaw, roll):
  """First half of depthViewTransWithConf_gpu: (r2 float64 (H, W), target index int32 (H, W), -1 = source takes no part)."""
  require_gpu(view_1)
  view_1 = view_1.contiguous()
  require_f32c(view_1)
  H, W = view_1.shape
  R = np.ascontiguousarray(_rotation(pitch, yaw, roll), dtype=np.float64)
  t = np.array([x0, y0, z0], dtype=np.float64)
  r2 = torch.empty((H, W), dtype=torch.float64, device=view_1.device)
  tgt = torch.empty((H, W), dtype=torch.int32, device=view_1.device)
  with torch.cuda.device_of(view_1):
    check(lib().mode_depth_view_project(ptr(view_1), ptr(_trig_device(H, W, str(view_1.device))), R.ctypes.data, t.ctypes.data, ptr(r2),
                                        ptr(tgt), H, W, stream_of(view_1)), 'mode_depth_view_project')
  return r2, tgt


def zbuffer_gpu(r2, target, conf_1):
  """Second half: the reference's z-buffer over (r2 float64, target int32, conf float32) triples of any shape -> (view_2, conf_2)."""
  require_gpu(r2, target, conf_1)
  r2, target, conf_1 = r2.contiguous(), target.contiguous(), conf_1.contiguous()
  n = r2.numel()
  view_2 = torch.empty(r2.shape, dtype=torch.float32, device=r2.device)
  conf_2 = torch.empty_like(view_2)
  ws = torch.empty(n, dtype=torch.int64, device=r2.device)
  with torch.cuda.device_of(r2):
    check(lib().mode_zbuffer(ptr(r2), ptr(target), ptr(conf_1), ptr(view_2), ptr(conf_2), ptr(ws), n, stream_of(r2)), 'mode_zbuffer')
  return view_2, conf_2


def depthViewTransWithConf(view_1, conf_1, y0, z0, x0, pitch, yaw, roll):
  """numpy (H, W) depth and confidence seen from camera 1 -> the same scene seen from a camera at (x0, y0, z0) rotated by
  (pitch, yaw, roll); float32 numpy out."""
  v = torch.from_numpy(np.ascontiguousarray(view_1, dtype=np.float32)).to(_DEV)
  c = torch.from_numpy(np.ascontiguousarray(conf_1, dtype=np.float32)).to(_DEV)
  v2, c2 = depthViewTransWithConf_gpu(v, c, y0, z0, x0, pitch, yaw, roll)
  return v2.cpu().numpy(), c2.cpu().numpy()


# ------------------------------------------------------------------------------------------------ disp2depth
CAM_PAIRS = {'12': 0, '13': 1, '14': 2, '23': 3, '24': 4, '34': 5}


def _baselines(dbname):
  """save_output_disparity_stage.py:108-113 (3D60 defines none)."""
  if dbname == 'Deep360':
    return np.array([1, 1, math.sqrt(2), math.sqrt(2), 1, 1]).astype(np.float32)
  if dbname == '3D60':
    raise ValueError('disp2depth: the reference defines no baselines for 3D60')
  return np.array([0.6 * math.sqrt(2), 0.6 * math.sqrt(2), 1.2, 1.2, 0.6 * math.sqrt(2), 0.6 * math.sqrt(2)]).astype(np.float32)


# camera 1's frame from the others (save_output_disparity_stage.py:136-158): pairs 13 and 14 are rotations of the Cassini image by the
# pitch below; pairs 23, 24 and 34 are depthViewTransWithConf(view, conf, y0, z0, x0, pitch, yaw, roll) with these arguments
_ROT_PITCH = {'13': 0.5 * math.pi, '14': 0.25 * math.pi}
_VIEW_POSES = {'23': (0, -math.sqrt(2) / 2, -math.sqrt(2) / 2, 0.75 * math.pi, 0, 0), '24': (0, -1, 0, 0.5 * math.pi, 0, 0),
               '34': (0, 1, 0, 0, 0, 0)}


def disp2depth_gpu(disp, conf_map, cam_pair, dbname='Deep360'):
  """disp, conf_map: (H, W) float32 device tensors -> (depth, conf) in the reference frame of camera 1, device tensors."""
  if cam_pair not in CAM_PAIRS:
    print("Error! Wrong Cam_pair!")
    return None
  require_gpu(disp, conf_map)
  disp = disp.contiguous()
  require_f32c(disp)
  H, W = disp.shape
  depth_l = torch.empty_like(disp)
  with torch.cuda.device_of(disp):
    check(lib().mode_disp2depth(ptr(disp), ptr(depth_l), H, W, float(_baselines(dbname)[CAM_PAIRS[cam_pair]]), stream_of(disp)), 'mode_disp2depth')
  if cam_pair == '12':
    return depth_l, conf_map
  if cam_pair in _ROT_PITCH:
    both = rotateCassini_gpu(torch.stack((depth_l, conf_map.to(depth_l.dtype))).unsqueeze(0), _ROT_PITCH[cam_pair], 0, 0)[0]
    return both[0], both[1]
  return depthViewTransWithConf_gpu(depth_l, conf_map, *_VIEW_POSES[cam_pair])


def disp2depth(disp, conf_map, cam_pair, dbname='Deep360'):
  """numpy in, numpy out (save_output_disparity_stage.py:105-160; `dbname` replaces the script's global args.dbname)."""
  d = torch.from_numpy(np.ascontiguousarray(disp, dtype=np.float32)).to(_DEV)
  c = torch.from_numpy(np.ascontiguousarray(conf_map, dtype=np.float32)).to(_DEV)
  out = disp2depth_gpu(d, c, cam_pair, dbname)
  if out is None:
    return None
  return out[0].cpu().numpy(), out[1].cpu().numpy()


# ------------------------------------------------------------------------------------------------ the multi-view hand-off
PAIRS = ('12', '13', '14', '23', '24', '34')  # the order of a frame's six pairs (CAM_PAIRS)
MV_CONF_PNG, MV_DEPTH_ONLY = CONSTANTS['MODE_MV_CONF_PNG'], CONSTANTS['MODE_MV_DEPTH_ONLY']
_frames_cache = _HF._LRU(8)  # (H, W, device, dbname) -> constant tables of mode_multiview_handoff (graph-pinned while captured);
#                              ('rig', rig, H, W, device) -> those of mode_multiview_rig_handoff for a utils.rig.CameraRig
_frames_lock = threading.Lock()


def _frames_tables(H, W, device, dbname):
  """(baselines float32 (6,) host, rotation grids (2, H, W, 2) device, trig device, 3 x (R, t) float64 (36,) host) -- the tables
  disp2depth_gpu uses for the six pairs, built by the same functions."""
  key = (H, W, str(device), dbname)
  with _frames_lock:
    hit = _frames_cache.get(key)
    if hit is not None:
      return hit
    baselines = np.ascontiguousarray(_baselines(dbname), dtype=np.float32)
    grids = torch.cat([_rotate_grid(H, W, float(_ROT_PITCH[p]), 0.0, 0.0, str(device)) for p in ('13', '14')]).contiguous()
    trig = _trig_device(H, W, str(device)).clone()
    xforms = []
    for p in ('23', '24', '34'):
      y0, z0, x0, pitch, yaw, roll = _VIEW_POSES[p]
      xforms += [np.ascontiguousarray(_rotation(pitch, yaw, roll), dtype=np.float64).ravel(), np.array([x0, y0, z0], dtype=np.float64)]
    entry = (baselines, grids, trig, np.ascontiguousarray(np.concatenate(xforms)))
    _frames_cache[key] = entry
    return entry


def _as_frames(t, what, rig=None):
  """(F, 6, H, W), (6F, 1, H, W) or (6F, H, W) -> a (F, 6, H, W) view; with a rig of P pairs, the same with 6 -> P (a (F, 1, H, W)
  tensor of a one-pair rig is both forms at once)."""
  if rig is not None:
    return _as_rig_frames(t, what, len(rig.pairs))
  if t.dim() == 4 and t.shape[1] == 6:
    return t
  if (t.dim() == 4 and t.shape[1] == 1) or t.dim() == 3:
    if t.shape[0] % 6:
      raise ValueError('disp2depth_frames_gpu: %s has %d maps, not six per frame' % (what, t.shape[0]))
    return t.view(t.shape[0] // 6, 6, t.shape[-2], t.shape[-1])
  raise ValueError('disp2depth_frames_gpu: %s of shape %s is not (F, 6, H, W), (6F, 1, H, W) or (6F, H, W)' % (what, tuple(t.shape)))


def _as_rig_frames(t, what, P):
  if t.dim() == 4 and t.shape[1] == P:
    return t
  if (t.dim() == 4 and t.shape[1] == 1) or t.dim() == 3:
    if t.shape[0] % P:
      raise ValueError('disp2depth_frames_gpu: %s has %d maps, not %d per frame of the rig' % (what, t.shape[0], P))
    return t.view(t.shape[0] // P, P, t.shape[-2], t.shape[-1])
  raise ValueError('disp2depth_frames_gpu: %s of shape %s is not (F, %d, H, W), (%dF, 1, H, W) or (%dF, H, W)' % (what, tuple(t.shape), P, P, P))


def _check_rig(rig, dbname, who):
  """A rig carries its own baselines and poses: it does not go together with a database name other than the default."""
  if rig is not None and dbname != 'Deep360':
    raise ValueError('%s: rig= and dbname=%r are two descriptions of the cameras; pass one (dbname selects among the reference\'s rigs, '
                     'utils.rig.CameraRig describes any)' % (who, dbname))


def _rig_tables(rig, H, W, device):
  """(mode_mv_pair records host, R, V, rotation grids (R, H, W, 2) device or None, trig device, V x (R, t) float64 host or None) of
  mode_multiview_rig_handoff for a utils.rig.CameraRig, built by the functions the single-map calls use and cached like _frames_tables."""
  key = ('rig', rig, H, W, str(device))
  with _frames_lock:
    hit = _frames_cache.get(key)
    if hit is not None:
      return hit
    records, R, V = rig.records()
    grids = [_rotate_grid(H, W, p.pose[0], p.pose[1], p.pose[2], str(device)) for p in rig.of_kind('rotate')]
    xforms = []
    for p in rig.of_kind('view'):
      y0, z0, x0, pitch, yaw, roll = p.pose
      xforms += [np.ascontiguousarray(_rotation(pitch, yaw, roll), dtype=np.float64).ravel(), np.array([x0, y0, z0], dtype=np.float64)]
    entry = (records, R, V, torch.cat(grids).contiguous() if grids else None, _trig_device(H, W, str(device)).clone(),
             np.ascontiguousarray(np.concatenate(xforms)) if xforms else None)
    _frames_cache[key] = entry
    return entry


_adjoint_cache = _HF._LRU(8)  # (H, W, device) -> adjoint lists of the two rotation grids (mode_multiview_handoff_bwd);
#                               (rig, H, W, device) -> those of a rig's R rotation grids (mode_multiview_rig_handoff_bwd)


def _bilinear_border_np(grid, Hs, Ws):
  """geom::bilinear_border (csrc/geometry_internal.h) on a (..., 2) float32 grid, operation for operation in numpy float32:
  (x0, y0, x1ok, y1ok, (nw, ne, sw, se))."""
  f32 = np.float32
  gx, gy = grid[..., 0].astype(f32), grid[..., 1].astype(f32)
  x = (gx + f32(1)) * f32(0.5) * f32(Ws - 1)
  y = (gy + f32(1)) * f32(0.5) * f32(Hs - 1)
  x = np.minimum(np.maximum(x, f32(0)), f32(Ws - 1))
  y = np.minimum(np.maximum(y, f32(0)), f32(Hs - 1))
  xf, yf = np.floor(x), np.floor(y)
  x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
  wx1, wy1 = x - xf, y - yf
  wx0, wy0 = f32(1) - wx1, f32(1) - wy1
  return x0, y0, x0 + 1 <= Ws - 1, y0 + 1 <= Hs - 1, (wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1)


def _grid_adjoint_np(grid, H, W):
  """The adjoint list of one (H, W, 2) sampling grid over an (H, W) source: for every source pixel the (target, weight) entries of the
  bilinear taps whose corner it is, sorted by source, then target, then corner (nw, ne, sw, se); corners outside the image are left
  out.  -> (counts per source int64 (H W,), target int32 (n,), weight float32 (n,))."""
  x0, y0, x1ok, y1ok, w = _bilinear_border_np(grid.reshape(H * W, 2), H, W)
  tgt = np.arange(H * W, dtype=np.int64)
  corners = ((y0 * W + x0, np.ones(H * W, dtype=bool)), (y0 * W + x0 + 1, x1ok), ((y0 + 1) * W + x0, y1ok),
             ((y0 + 1) * W + x0 + 1, x1ok & y1ok))
  src = np.concatenate([s[ok] for s, ok in corners])
  t = np.concatenate([tgt[ok] for _, ok in corners])
  c = np.concatenate([np.full(int(ok.sum()), k, dtype=np.int64) for k, (_, ok) in enumerate(corners)])
  wt = np.concatenate([w[k][ok] for k, (_, ok) in enumerate(corners)])
  order = np.lexsort((c, t, src))
  return np.bincount(src, minlength=H * W), t[order].astype(np.int32), wt[order].astype(np.float32)


def _frames_adjoint(H, W, device):
  """(rowptr int32 (2, H W + 1), target int32 (n,), weight float32 (n,)) on the device: the adjoint lists of the rotation grids of
  pairs 13 and 14 in CSR form, the second grid's entries behind the first's (rowptr[1, 0] == rowptr[0, H W]; n <= 8 H W).  Built once
  per (H, W, device) on the host from the cached grids."""
  key = (H, W, str(device))
  with _frames_lock:
    hit = _adjoint_cache.get(key)
    if hit is not None:
      return hit
    rowptr, targets, weights, base = [], [], [], 0
    for p in ('13', '14'):
      grid = _rotate_grid(H, W, float(_ROT_PITCH[p]), 0.0, 0.0, str(device))[0].cpu().numpy()
      counts, t, w = _grid_adjoint_np(grid, H, W)
      rowptr.append(base + np.concatenate(([0], np.cumsum(counts))))
      targets.append(t)
      weights.append(w)
      base += len(t)
    rowptr = np.stack(rowptr)
    # the kernel cannot report a malformed list (it clamps and skips), so the only producer checks what it hands over
    if rowptr[0, 0] != 0 or rowptr[1, 0] != rowptr[0, -1] or rowptr[1, -1] != base or (np.diff(rowptr.ravel()) < 0).any() or base > 8 * H * W:
      raise RuntimeError('_frames_adjoint: inconsistent adjoint lists for %d x %d' % (H, W))
    entry = (torch.from_numpy(rowptr.astype(np.int32)).to(device), torch.from_numpy(np.concatenate(targets)).to(device),
             torch.from_numpy(np.concatenate(weights)).to(device))
    _adjoint_cache[key] = entry
    return entry


def _rig_adjoint(rig, H, W, device):
  """_frames_adjoint for the R rotation grids of a rig, in pair order: (rowptr int32 (R, H W + 1) or None, target, weight)."""
  key = (rig, H, W, str(device))
  with _frames_lock:
    hit = _adjoint_cache.get(key)
    if hit is not None:
      return hit
    rowptr, targets, weights, base = [], [np.zeros(0, np.int32)], [np.zeros(0, np.float32)], 0
    for p in rig.of_kind('rotate'):
      grid = _rotate_grid(H, W, p.pose[0], p.pose[1], p.pose[2], str(device))[0].cpu().numpy()
      counts, t, w = _grid_adjoint_np(grid, H, W)
      rowptr.append(base + np.concatenate(([0], np.cumsum(counts))))
      targets.append(t)
      weights.append(w)
      base += len(t)
    if rowptr:
      rowptr = np.stack(rowptr)
      # as _frames_adjoint: the only producer checks what it hands over
      if (rowptr[0, 0] != 0 or (rowptr[1:, 0] != rowptr[:-1, -1]).any() or rowptr[-1, -1] != base or (np.diff(rowptr.ravel()) < 0).any() or
          base > 4 * len(rowptr) * H * W or base >= 2 ** 31):
        raise RuntimeError('_rig_adjoint: inconsistent adjoint lists for %d x %d' % (H, W))
      rowptr = torch.from_numpy(rowptr.astype(np.int32)).to(device)
    else:
      rowptr = None
    entry = (rowptr, torch.from_numpy(np.concatenate(targets)).to(device), torch.from_numpy(np.concatenate(weights)).to(device))
    _adjoint_cache[key] = entry
    return entry


def _optr(t):
  return None if t is None else ptr(t)


def _host(a):
  return None if a is None else a.ctypes.data


def _rig_handoff_fwd(disp, conf, rig, conf_png, depth_only):
  """disp, conf (F, P, H, W) contiguous -> (out, the key planes (F, V, H, W) int64), on mode_multiview_rig_handoff."""
  F, P, H, W = disp.shape
  records, R, V, grids, trig, xforms = _rig_tables(rig, H, W, disp.device)
  out = torch.empty((F, P if depth_only else 2 * P, H, W), dtype=torch.float32, device=disp.device)
  ws = torch.empty(lib().mode_multiview_rig_handoff_workspace_bytes(F, V, H, W) // 8, dtype=torch.int64, device=disp.device)
  flags = (MV_CONF_PNG if conf_png else 0) | (MV_DEPTH_ONLY if depth_only else 0)
  with torch.cuda.device_of(disp):
    check(lib().mode_multiview_rig_handoff(ptr(disp), ptr(conf), F, P, H, W, records.ctypes.data, R, _optr(grids), ptr(trig), V, _host(xforms),
                                           flags, ptr(out), ptr(ws) if ws.numel() else None, stream_of(disp)), 'mode_multiview_rig_handoff')
  return out, ws.view(F, V, H, W)


def _handoff_fwd(disp, conf, dbname, conf_png, depth_only, rig=None):
  """disp, conf (F, 6, H, W) contiguous -> (out, the key planes (F, 3, H, W) int64 the launches leave behind)."""
  if rig is not None:
    return _rig_handoff_fwd(disp, conf, rig, conf_png, depth_only)
  F, _, H, W = disp.shape
  baselines, grids, trig, xforms = _frames_tables(H, W, disp.device, dbname)
  out = torch.empty((F, 6 if depth_only else 12, H, W), dtype=torch.float32, device=disp.device)
  ws = torch.empty(lib().mode_multiview_handoff_workspace_bytes(F, H, W) // 8, dtype=torch.int64, device=disp.device)
  flags = (MV_CONF_PNG if conf_png else 0) | (MV_DEPTH_ONLY if depth_only else 0)
  with torch.cuda.device_of(disp):
    check(lib().mode_multiview_handoff(ptr(disp), ptr(conf), F, H, W, baselines.ctypes.data, ptr(grids), ptr(trig), xforms.ctypes.data, flags,
                                       ptr(out), ptr(ws), stream_of(disp)), 'mode_multiview_handoff')
  return out, ws.view(F, 3, H, W)


def _rig_handoff_bwd(disp, gout, keys, rig, depth_only, conf_grad):
  """disp2depth_frames_bwd for a rig, on mode_multiview_rig_handoff_bwd / _bwd_full."""
  require_gpu(disp, gout, keys)
  disp, gout, keys = _as_frames(disp.contiguous(), 'disp', rig), gout.contiguous(), keys.contiguous()
  require_f32c(disp, gout)
  F, P, H, W = disp.shape
  records, R, V, _, trig, xforms = _rig_tables(rig, H, W, disp.device)
  if P != len(rig.pairs) or tuple(gout.shape) != (F, P if depth_only else 2 * P, H, W) or keys.dtype != torch.int64 or keys.numel() != V * F * H * W:
    raise ValueError('disp2depth_frames_bwd: disp %s, gout %s and keys %s %s do not belong together for a rig of %d pairs, %d of them view '
                     'transforms' % (tuple(disp.shape), tuple(gout.shape), keys.dtype, tuple(keys.shape), len(rig.pairs), V))
  rowptr, target, weight = _rig_adjoint(rig, H, W, disp.device)
  kptr = ptr(keys) if keys.numel() else None
  gdisp = torch.empty_like(disp)
  if conf_grad and not depth_only:
    gconf = torch.empty_like(disp)
    with torch.cuda.device_of(disp):
      check(lib().mode_multiview_rig_handoff_bwd_full(ptr(disp), ptr(gout), kptr, F, P, H, W, records.ctypes.data, R, ptr(trig), V, _host(xforms),
                                                      _optr(rowptr), ptr(target), ptr(weight), target.numel(), 0, ptr(gdisp), ptr(gconf),
                                                      stream_of(disp)), 'mode_multiview_rig_handoff_bwd_full')
    return gdisp, gconf
  with torch.cuda.device_of(disp):
    check(lib().mode_multiview_rig_handoff_bwd(ptr(disp), ptr(gout), kptr, F, P, H, W, records.ctypes.data, R, ptr(trig), V, _host(xforms),
                                               _optr(rowptr), ptr(target), ptr(weight), target.numel(), MV_DEPTH_ONLY if depth_only else 0,
                                               ptr(gdisp), stream_of(disp)), 'mode_multiview_rig_handoff_bwd')
  return (gdisp, None) if conf_grad else gdisp


def disp2depth_frames_bwd(disp, gout, keys, dbname='Deep360', depth_only=False, conf_grad=False, rig=None):
  """The gradient of disp2depth_frames_gpu's depth channels with respect to disp (mode_multiview_handoff_bwd): disp (F, 6, H, W) or one
  of the views the forward takes, gout the gradient of the output in its layout, keys the key planes of the forward on the same disp (return_keys) -> gdisp (F, 6, H, W).
  The confidence channels of gout are not read.  conf_grad=True (the forward with conf_png=False: q the identity) -> (gdisp, gconf):
  the gradient with respect to the confidence maps as well, from the confidence channels of gout, in the same two launches
  (mode_multiview_handoff_bwd_full; gdisp has the same bits; gconf is None with depth_only, which has no confidence channels).
  Bit-repeatable: sums over the cached adjoint lists in their stored order, no atomics.
  rig: a utils.rig.CameraRig of P pairs, V of them view transforms, as the forward took it: 6 -> P above, and keys (F, V, H, W)."""
  _check_rig(rig, dbname, 'disp2depth_frames_bwd')
  if rig is not None:
    return _rig_handoff_bwd(disp, gout, keys, rig, depth_only, conf_grad)
  require_gpu(disp, gout, keys)
  disp, gout, keys = _as_frames(disp.contiguous(), 'disp'), gout.contiguous(), keys.contiguous()
  require_f32c(disp, gout)
  F, six, H, W = disp.shape
  if six != 6 or tuple(gout.shape) != (F, 6 if depth_only else 12, H, W) or keys.dtype != torch.int64 or keys.numel() != 3 * F * H * W:
    raise ValueError('disp2depth_frames_bwd: disp %s, gout %s and keys %s %s do not belong together' %
                     (tuple(disp.shape), tuple(gout.shape), keys.dtype, tuple(keys.shape)))
  baselines, _, trig, xforms = _frames_tables(H, W, disp.device, dbname)
  rowptr, target, weight = _frames_adjoint(H, W, disp.device)
  gdisp = torch.empty_like(disp)
  if conf_grad and not depth_only:
    gconf = torch.empty_like(disp)
    with torch.cuda.device_of(disp):
      check(lib().mode_multiview_handoff_bwd_full(ptr(disp), ptr(gout), ptr(keys), F, H, W, baselines.ctypes.data, ptr(trig),
                                                  xforms.ctypes.data, ptr(rowptr), ptr(target), ptr(weight), target.numel(), 0, ptr(gdisp),
                                                  ptr(gconf), stream_of(disp)), 'mode_multiview_handoff_bwd_full')
    return gdisp, gconf
  with torch.cuda.device_of(disp):
    check(lib().mode_multiview_handoff_bwd(ptr(disp), ptr(gout), ptr(keys), F, H, W, baselines.ctypes.data, ptr(trig), xforms.ctypes.data,
                                           ptr(rowptr), ptr(target), ptr(weight), target.numel(), MV_DEPTH_ONLY if depth_only else 0,
                                           ptr(gdisp), stream_of(disp)), 'mode_multiview_handoff_bwd')
  return (gdisp, None) if conf_grad else gdisp


class _HandoffFunction(torch.autograd.Function):
  """disp2depth_frames_gpu with a gradient for disp (and, with conf_grad, for conf): the forward's launches and bits, disp and the key
  planes kept for the backward."""

  @staticmethod
  def forward(ctx, disp, conf, dbname, conf_png, depth_only, conf_grad=False, rig=None):
    out, keys = _handoff_fwd(disp, conf, dbname, conf_png, depth_only, rig)
    ctx.save_for_backward(disp, keys)
    ctx.dbname, ctx.depth_only, ctx.conf_grad, ctx.rig = dbname, depth_only, conf_grad, rig
    ctx.mark_non_differentiable(keys)
    return out, keys

  @staticmethod
  @once_differentiable  # (the kernel has no second derivative: create_graph=True raises instead of returning a detached gradient)
  def backward(ctx, gout, _gkeys):
    disp, keys = ctx.saved_tensors
    if ctx.conf_grad and not ctx.depth_only and ctx.needs_input_grad[1]:
      gdisp, gconf = disp2depth_frames_bwd(disp, gout, keys, ctx.dbname, conf_grad=True, rig=ctx.rig)
      return (gdisp if ctx.needs_input_grad[0] else None), gconf, None, None, None, None, None
    gdisp = disp2depth_frames_bwd(disp, gout, keys, ctx.dbname, ctx.depth_only, rig=ctx.rig) if ctx.needs_input_grad[0] else None
    return gdisp, None, None, None, None, None, None


def disp2depth_frames_gpu(disp, conf, dbname='Deep360', conf_png=False, depth_only=False, return_keys=False, conf_grad=False, rig=None):
  """The six pairs of F frames at once: disp, conf (F, 6, H, W) float32 device tensors (pair order PAIRS; (6F, 1, H, W) and
  (6F, H, W) are taken as views) -> (F, 12, H, W) with out[f, 2p], out[f, 2p + 1] = disp2depth_gpu(disp[f, p], conf[f, p], PAIRS[p],
  dbname) -- ModeFusion's channel interleave -- bit for bit, in three launches (mode_multiview_handoff).  conf_png: every confidence
  as the reference's 8-bit PNG export reads back, q(c) = float32(float64(clip(rint(c * 255), 0, 255)) / 255).  depth_only:
  (F, 6, H, W) of the depths alone (the input of Baseline).

  Differentiable in disp (disp2depth_frames_bwd): the depth channels pass their gradient through the sine rule, the bilinear taps
  of the rotation and, for the view-transformed pairs, to the z-buffer's winner alone.  By default the confidence gets no gradient
  (None for conf).  conf_grad=True: conf gets the gradient of the confidence channels too -- they are linear in it: the copy, the
  rotation's taps, the winner's pick -- from the same two launches (mode_multiview_handoff_bwd_full).  That needs q the identity:
  with conf_png=True it raises ValueError (the 8-bit rounding is piecewise constant); with depth_only there are no confidence
  channels and conf gets None.  return_keys: (out, keys) with the forward's z-buffer key planes (F, 3, H, W) int64 (layout:
  csrc/geometry_internal.h).

  rig: a utils.rig.CameraRig instead of a database name (passing both is a ValueError).  disp, conf are then (F, P, H, W) in the rig's
  pair order ((P F, 1, H, W) and (P F, H, W) are taken as views), the result (F, 2P, H, W) -- (F, P, H, W) with depth_only -- and the
  key planes (F, V, H, W) for its V view-transformed pairs, in pair order: every plane has the bits of the single-map calls for its
  pair (mode_disp2depth, then rotateCassini_gpu or depthViewTransWithConf_gpu with the pair's pose), in three launches, or one when the
  rig has no view-transformed pair (mode_multiview_rig_handoff).  Everything above holds with 6 -> P.  rig=None is the path above,
  untouched."""
  _check_rig(rig, dbname, 'disp2depth_frames_gpu')
  if conf_grad and conf_png:
    raise ValueError('disp2depth_frames_gpu: conf_grad=True needs conf_png=False: the 8-bit PNG rounding of the confidence is piecewise '
                     'constant and passes no gradient')
  require_gpu(disp, conf)
  disp, conf = _as_frames(disp.contiguous(), 'disp', rig), _as_frames(conf.contiguous(), 'conf', rig)
  require_f32c(disp, conf)
  if disp.shape != conf.shape or disp.device != conf.device:
    raise ValueError('disp2depth_frames_gpu: disp %s and conf %s differ' % (tuple(disp.shape), tuple(conf.shape)))
  if torch.is_grad_enabled() and (disp.requires_grad or conf.requires_grad):
    out, keys = _HandoffFunction.apply(disp, conf, dbname, bool(conf_png), bool(depth_only), bool(conf_grad), rig)
  else:
    out, keys = _handoff_fwd(disp, conf, dbname, conf_png, depth_only, rig)
  return (out, keys) if return_keys else out


def conf_png_np(c):
  """The q rule on the host (numpy float32 in and out): the 8-bit PNG round trip of the reference's confidence export."""
  c = np.asarray(c, dtype=np.float32)
  return (np.clip(np.rint(c * np.float32(255)), 0, 255).astype(np.float64) / 255.0).astype(np.float32)
