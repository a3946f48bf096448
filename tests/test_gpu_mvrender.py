"""GPU (-m gpu): the novel-view rendering of DESIGN 29 -- HF.mv_render (csrc/mv_render.hip) and ModeMultiView.render_views -- against the
float64 restatement of tests/mvrender_ref.py.

hit and index are exact: the kernel computes rho, u, v, u_r and v_r in fp64 as the restatement does, the minima are integer minima, and
tests/test_mvrender_host.py asserts on the restatement that no landing pixel, no edge of validity, no pair of competing ranges and no
comparison with (1 + tol) zn of the cases sits within 1e-9 of its kink.  range: the +inf pattern exactly, the finite values within one
fp32 ulp.  The splat's colours are copies: torch.equal to the image gathered by the restatement's index.  The resampled colours by
DESIGN 24's bound: the yardstick is the float32 restatement's own error against float64 (max over ALL elements, relative to
max|out64|), never below 2^-23 of it, and the kernel may take 4 times it.

Measured ratios on an MI355X: see DESIGN 29."""
import numpy as np
import pytest
import torch

import mvphoto_ref as M
import mvpose_ref as P
import mvrender_ref as R

from mode_hip import functional as HF
from utils import geometry
from utils.rig import CameraRig

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ALL = R.CASES + (R.SPHERES,)
IDS = ['x'.join(str(v) for v in c) for c in ALL]


@pytest.fixture(autouse=True)
def _stop_at_a_gpu_fault():
  """As tests/test_gpu_guard_bands.py: if the device no longer answers after a test, the session ends there."""
  yield
  try:
    torch.cuda.synchronize()
  except RuntimeError as e:
    pytest.exit('the GPU reported an error after this test; nothing more is started on it: %s' % e, returncode=3)


def _render(image, depth, poses, **kw):
  """-> (out, range, hit, index) on the CPU through the public entry."""
  out, rng, hit, index = HF.mv_render(image.to(DEV), depth.to(DEV), poses, return_range=True, return_hit=True, return_index=True, **kw)
  F, C, H, W = image.shape
  T = hit.shape[1]
  assert out.shape == (F, T, C, H, W) and out.dtype == torch.float32 and hit.shape == (F, T, H, W) and hit.dtype == torch.uint8
  assert rng.shape == hit.shape and rng.dtype == torch.float32 and index.shape == hit.shape and index.dtype == torch.int32
  assert all(x.is_cuda and not x.requires_grad for x in (out, rng, hit, index))
  return out.cpu(), rng.cpu(), hit.cpu(), index.cpu()


def _one_ulp(got, want):
  """The +inf pattern exactly; finite values within one fp32 ulp (as integers, the bit patterns of positive floats are consecutive)."""
  inf = torch.isinf(want)
  assert torch.equal(torch.isinf(got), inf) and bool((got[inf] > 0).all()) and not bool(torch.isnan(got).any())
  steps = (got[~inf].view(torch.int32) - want[~inf].view(torch.int32)).abs()
  return int(steps.max()) if steps.numel() else 0


def _gathered(image, index):
  """image (F, C, H, W), index (F, T, H, W) -> (F, T, C, H, W): image(f, c, index), 0 where index is -1."""
  F, C, H, W = image.shape
  T = index.shape[1]
  idx = index.long().clamp(min=0).reshape(F, 1, T * H * W).expand(F, C, -1)
  got = image.reshape(F, C, H * W).gather(2, idx).reshape(F, C, T, H, W).permute(0, 2, 1, 3, 4)
  return torch.where((index >= 0).unsqueeze(2), got, torch.zeros(())).contiguous()


def _check(tag, image, depth, poses, tol, fill, want64, want32=None, C=3):
  """One setting, both modes, against the restatement (want64: RESAMPLE in float64; want32: the same in float32 or None for no colour
  comparison of the resampled output) -> the ratio of the resampled colours or None."""
  img = R.channels(image, C)
  out, rng, hit, index = _render(img, depth, poses, tol=tol, fill=fill, mode='splat')
  assert torch.equal(hit, want64['hit'] & (R.DIRECT | R.FILLED)), (tag, tol, fill, int((hit != want64['hit'] & (R.DIRECT | R.FILLED)).sum()))
  assert torch.equal(index, want64['index']), (tag, tol, fill, int((index != want64['index']).sum()))
  ulps = _one_ulp(rng, want64['range'])
  assert ulps <= 1
  assert torch.equal(out.view(torch.int32), _gathered(img, want64['index']).view(torch.int32)), (tag, tol, fill, C)
  out_r, rng_r, hit_r, index_r = _render(img, depth, poses, tol=tol, fill=fill, mode='resample')
  assert torch.equal(hit_r, want64['hit']), (tag, tol, fill, int((hit_r != want64['hit']).sum()))
  assert torch.equal(index_r, index) and torch.equal(rng_r.view(torch.int32), rng.view(torch.int32))
  splat_value = hit_r & R.RESAMPLED == 0
  assert torch.equal(out_r.permute(0, 1, 3, 4, 2)[splat_value], out.permute(0, 1, 3, 4, 2)[splat_value])  # beyond the poles, and NONE
  ratio = None
  if want32 is not None:
    yard, scale = M.yardstick(want32['out'], want64['out'])
    err = M.error(out_r, want64['out'], scale)
    ratio = err / yard
    print('  %s tol %g fill %d C %d: %d of %d seen, %d resampled; range within %d ulp; max|out64| %.3e, error %.3e, yardstick %.3e of it, '
          'ratio %.2f' % (tag, tol, fill, C, int((hit_r != 0).sum()), hit_r.numel(), int((hit_r & R.RESAMPLED != 0).sum()), ulps, scale, err,
                          yard, ratio))
    assert scale > 0 and bool(torch.isfinite(out_r).all()) and err <= 4 * yard, (tag, tol, fill, err, yard)
  return ratio


# ------------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize('case', ALL, ids=IDS)
def test_render_equals_the_float64_restatement(case):
  image, depth, poses = R.make_case(case)
  for tol in R.TOLS:
    for fill in R.FILLS:
      _check(str(case), image, depth, poses, tol, fill, R.reference(case, tol, fill), R.reference(case, tol, fill, dtype=torch.float32))
  for C in (1, 4):
    _check(str(case), image, depth, poses, 0.05, 1, R.reference(case, 0.05, 1, C=C), R.reference(case, 0.05, 1, dtype=torch.float32, C=C), C=C)
  # the defaults: tol 0.05, fill 1, resample, and nothing but out
  only = HF.mv_render(image.to(DEV), depth.to(DEV), poses)
  assert torch.is_tensor(only) and torch.equal(only.cpu(), _render(image, depth, poses)[0])


def test_spoilt_depths_never_own_a_pixel():
  """NaN, +Inf, 0 and a negative depth at single pixels, corners included: invalid for every view, so no target pixel names them, and
  everything is the restatement's, which leaves them out."""
  case = R.CASES[0]
  image, depth, poses = R.make_case(case)
  depth = depth.clone()
  F, H, W, T = case
  spots = ((0, 3, 5, float('nan')), (0, 20, 10, 0.0), (1, 7, 7, -2.0), (1, 30, 20, float('inf')), (1, 0, 0, float('nan')), (0, 39, 23, 0.0),
           (0, 0, 23, float('inf')), (1, 39, 0, -1.0))
  for f, h, w, bad in spots:
    depth[f, h, w] = bad
  for fill in R.FILLS:
    want = R.render(image, depth, poses, 0.05, fill, R.RESAMPLE)
    _check('spoilt depths', image, depth, poses, 0.05, fill, want, R.render(image, depth, poses, 0.05, fill, R.RESAMPLE, torch.float32))
    index = _render(image, depth, poses, fill=fill)[3]
    for f, h, w, _ in spots:
      assert not bool((index[f] == h * W + w).any()), (f, h, w)
  nothing = _render(image, torch.full_like(depth, float('nan')), poses)
  assert not bool(nothing[0].any()) and bool((nothing[1] == float('inf')).all()) and not bool(nothing[2].any()) and bool((nothing[3] == -1).all())


def test_eleven_views_run_in_two_chunks():
  case = R.CASES[1]
  image, depth, _ = R.make_case(case)
  twist = torch.tensor([[v * (1 + 0.15 * k) for v in R.TW[k % 3]] for k in range(11)], dtype=torch.float64)
  poses = P.twisted(torch.eye(3, 4, dtype=torch.float64).reshape(1, 12).repeat(11, 1), twist).numpy()
  whole = _render(image, depth, poses)
  first, second = _render(image, depth, poses[:8]), _render(image, depth, poses[8:])
  assert whole[2].shape[1] == 11 and int((whole[2] != 0).sum()) > 0
  for w, a, b in zip(whole, first, second):
    assert torch.equal(w.view(torch.uint8), torch.cat([a, b], 1).contiguous().view(torch.uint8))
  only = HF.mv_render(image.to(DEV), depth.to(DEV), poses, mode='splat')
  assert only.shape == (1, 11, 3) + tuple(depth.shape[1:])


def test_the_four_dimensional_layout_and_the_pose_forms():
  case = R.CASES[2]
  image, depth, poses = R.make_case(case)
  a = _render(image, depth, poses)
  for d, p in ((depth.unsqueeze(1), torch.from_numpy(poses).reshape(-1, 3, 4)), (depth, poses.tolist()), (depth, torch.from_numpy(poses).to(DEV)),
               (depth.unsqueeze(1), torch.from_numpy(poses).clone().requires_grad_(True))):
    b = _render(image, d, p)
    for x, y in zip(a, b):
      assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
  img, dep = image.to(DEV), depth.to(DEV)
  got = HF.mv_render(img.requires_grad_(True), dep.clone().requires_grad_(True), poses)  # no autograd: the inputs are detached
  assert not got.requires_grad and torch.equal(got.cpu(), a[0])
  rng, index = HF.mv_render(img, dep, poses, return_range=True, return_index=True)[1:]
  assert torch.equal(rng.cpu().view(torch.int32), a[1].view(torch.int32)) and torch.equal(index.cpu(), a[3])
  for bad in (np.zeros((2, 13)), np.zeros(12), np.zeros((2, 4, 3)), np.zeros((0, 12))):
    with pytest.raises(ValueError, match=r'poses must be \(T, 12\) or \(T, 3, 4\)|no target view'):
      HF.mv_render(img, dep, bad)
  for kw, words in (({'tol': -0.1}, 'tol'), ({'fill': 2}, 'fill'), ({'mode': 'nearest'}, 'mode')):
    with pytest.raises(ValueError, match=words):
      HF.mv_render(img, dep, poses, **kw)
  with pytest.raises(ValueError, match='image must be'):
    HF.mv_render(torch.cat([img, img], 1), dep, poses)
  with pytest.raises(ValueError, match='a depth map of shape'):
    HF.mv_render(img, dep[:, :-1], poses)


def test_two_calls_and_a_side_stream_are_bit_equal():
  case = R.CASES[3]
  image, depth, poses = R.make_case(case)
  a = _render(image, depth, poses)
  b = _render(image, depth, poses)
  side = torch.cuda.Stream(device=DEV)
  side.wait_stream(torch.cuda.current_stream(DEV))
  with torch.cuda.stream(side):
    c = _render(image, depth, poses)
  side.synchronize()
  for x, y, z in zip(a, b, c):
    assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)) and torch.equal(x.view(torch.uint8), z.view(torch.uint8))


# ------------------------------------------------------------------------------------------------------------------ the model
def test_render_views_is_the_hand_assembled_call():
  """ModeMultiView(rig = pairs 12, 13) at 64 x 32: render_views is HF.mv_render of the frame's reference panorama through forward()'s
  depth; it runs in eval mode whatever mode the module is in and leaves the modes as they were; erp=True is cassini2Equirec by hand."""
  import test_gpu_rig as TR
  rig = CameraRig.deep360().subset(('12', '13'))
  net, maxdepth, H, W = TR._tiny_net(rig)
  assert (H, W) == (64, 32) and rig.reference_panorama() == 0
  frames_u8 = TR._u8_frames(2, 4, H, W, 61)
  normalised = TR._host_normalised(frames_u8)
  poses = R.poses_of(3)
  rendered, rng, hit = net.render_views(normalised, poses)
  depth = net(normalised)
  want = HF.mv_render(normalised[:, 0], depth, poses, return_range=True, return_hit=True)
  assert rendered.shape == (2, 3, 3, H, W) and rng.shape == hit.shape == (2, 3, H, W) and not rendered.requires_grad
  assert torch.equal(rendered, want[0]) and torch.equal(rng.view(torch.int32), want[1].view(torch.int32)) and torch.equal(hit, want[2])
  assert 0 < int((hit != 0).sum())
  again = net.render_views(frames_u8, poses, mode='splat', fill=0, tol=0.0)  # 8-bit frames, and the keywords pass through
  by_hand = HF.mv_render(normalised[:, 0], depth, poses, mode='splat', fill=0, tol=0.0, return_range=True, return_hit=True)
  assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(again, by_hand))
  net.train()
  net.disparity.eval()
  training = net.render_views(normalised, poses)
  assert net.training and net.fusion.training and not net.disparity.training
  assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(training, (rendered, rng, hit)))
  net.eval()
  e_rendered, e_rng, e_hit = net.render_views(normalised, poses, erp=True)
  assert e_rendered.shape == (2, 3, 3, W, H) and e_rng.shape == (2, 3, W, H)
  for t in range(3):
    assert torch.equal(e_rendered[:, t], geometry.cassini2Equirec(rendered[:, t].contiguous()))
    by_hand = geometry.cassini2Equirec(rng[:, t].unsqueeze(1).contiguous())  # (+inf where nothing is seen: compared as bits)
    assert torch.equal(e_rng[:, t].view(torch.int32), by_hand.view(torch.int32))
  assert torch.equal(e_hit, hit)
