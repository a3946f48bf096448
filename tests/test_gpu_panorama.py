"""GPU: scoring of fused depth in the ERP domain (csrc/erp_metrics.hip, utils.panorama, ModeMultiView.evaluate).

The fused per-frame entry is checked bit for bit against the path it replaces (cassini2Equirec twice, `<=`, masked_metrics per
frame), for batch independence and repeatability (second call, side stream, graph replay), against an independent float64 evaluation
on the CPU (tests/panorama_ref.py) with bounds measured from torch's own fp32 evaluation of the same chain, on its selection edge
cases, and through ModeMultiView.evaluate.  mode_bicubic_up2 is checked against torch's float64 F.interpolate."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import panorama_ref as R
import recipe

import mode_hip
import models
from mode_hip import functional as HF
from utils import evaluation as E
from utils import geometry as HG
from utils import panorama

DEV = 'cuda:0'
SIZES = [(64, 32), (50, 25), (1024, 512)]  # 50 x 25: n % 4 != 0, so odd frames start off the 16-byte grid
EXTRA = dict(px=(1,), d1=((3, 0.05),))  # the other two threshold kinds ride along in the statistic vector


def _bits(t):
  return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).tobytes()


def _assert_gt_clear_of_maxdepth(gt, maxdepth=R.MAXDEPTH):
  """No ERP pixel's float64 gt within a relative 1e-4 of maxdepth: the fp32 and float64 selections are the same set."""
  ge64 = R.c2e(gt, torch.float64)
  assert int(((ge64 - maxdepth).abs() <= 1e-4 * maxdepth).sum()) == 0
  return ge64


def _unfused(p, g, maxdepth=R.MAXDEPTH, **kw):
  """What a user composes by hand: per frame two cassini2Equirec calls, the aten `<=` and masked_metrics."""
  pe, ge = HG.cassini2Equirec(p.unsqueeze(1)), HG.cassini2Equirec(g.unsqueeze(1))
  stats = [HF.masked_metrics(pe[f], ge[f], ge[f] <= maxdepth, **kw) for f in range(p.shape[0])]
  return stats, pe, ge


@pytest.mark.gpu
@pytest.mark.parametrize('frames', [1, 2, 5])
@pytest.mark.parametrize('size', SIZES)
def test_fused_rows_are_the_unfused_path_bit_for_bit(size, frames):
  H, W = size
  pred, gt = R.make_inputs(frames, H, W)
  _assert_gt_clear_of_maxdepth(gt)
  p, g = pred.to(DEV), gt.to(DEV)
  grid = HG._c2e_grid(W, H, DEV)
  kw = dict(ratio=R.RATIOS, **EXTRA)
  want, want_pe, want_ge = _unfused(p, g, **kw)
  stats, pe, ge = HF.erp_depth_metrics(p, g, grid, R.MAXDEPTH, return_erp=True, **kw)
  assert stats.shape == (frames, HF.METRICS_COUNT) and stats.dtype == torch.float64 and stats.is_cuda
  assert pe.shape == ge.shape == (frames, W, H)
  assert _bits(pe) == _bits(want_pe) and _bits(ge) == _bits(want_ge)
  got = stats.cpu().numpy()
  for f in range(frames):
    assert got[f].tobytes() == want[f].tobytes(), (f, got[f], want[f])
  sel = got[:, 0] / (H * W)
  assert (sel > 0.85).all() and (sel < 0.95).all()  # about 91 % selected
  assert got[-1, 2] < got[-1, 0]  # the pred = -1 block: selected, outside the log terms
  # without the ERP outputs: the same statistics
  assert _bits(HF.erp_depth_metrics(p, g, grid, R.MAXDEPTH, **kw)) == _bits(stats)
  # the reference's rows (test_fusion.py:93-100 at batch size 1)
  rows, pe2, ge2 = panorama.erp_depth_metrics(p.unsqueeze(1), g, R.MAXDEPTH, return_erp=True)
  assert rows.shape == (frames, 8) and rows.dtype == np.float64
  assert _bits(pe2) == _bits(want_pe) and _bits(ge2) == _bits(want_ge)
  for f in range(frames):
    ref = np.array(E.depth_metrics(want_pe[f], want_ge[f], want_ge[f] <= R.MAXDEPTH))
    assert ref.dtype == np.float64 and rows[f].tobytes() == ref.tobytes(), (f, rows[f], ref)
  assert np.isfinite(rows).all()
  assert _bits(panorama.erp_depth_metrics(p, g.unsqueeze(1))) == _bits(rows)


@pytest.mark.gpu
@pytest.mark.parametrize('size', [(50, 25), (1024, 512)])
def test_rows_depend_on_their_frame_alone_and_repeat(size):
  H, W = size
  pred, gt = R.make_inputs(5, H, W)
  p, g = pred.to(DEV), gt.to(DEV)
  grid = HG._c2e_grid(W, H, DEV)
  kw = dict(ratio=R.RATIOS, **EXTRA)
  five = HF.erp_depth_metrics(p, g, grid, R.MAXDEPTH, **kw)
  for f in range(5):
    one = HF.erp_depth_metrics(p[f:f + 1].clone(), g[f:f + 1].clone(), grid, R.MAXDEPTH, **kw)
    assert _bits(one[0]) == _bits(five[f]), f
  again = HF.erp_depth_metrics(p, g, grid, R.MAXDEPTH, **kw)
  side = torch.cuda.Stream(DEV)
  side.wait_stream(torch.cuda.current_stream(DEV))
  with torch.cuda.stream(side):
    on_side = HF.erp_depth_metrics(p, g, grid, R.MAXDEPTH, **kw)
  torch.cuda.current_stream(DEV).wait_stream(side)
  torch.cuda.synchronize()
  assert _bits(again) == _bits(five) == _bits(on_side)
  assert HF.erp_depth_metrics(p[:0], g[:0], grid, R.MAXDEPTH, **kw).shape == (0, HF.METRICS_COUNT)


# Seeds of the float64 comparison, one per size: the FIRST seed from 2022 on whose inputs meet two conditions that involve the CPU
# references only, never the code under test: at most 0.1 % of the selected pixels have a float64 ratio within 1e-4 (relative) of a
# delta_acc threshold (asserted in the test), and every fp32-reference distance from float64 -- the yardstick of the test -- was at
# least 2^-25 relative (half an fp32 ulp) where the seeds were picked: an fp32 result that lands closer to float64 than its own
# rounding step is a coincidence, and eight times a coincidence bounds nothing.  (The second condition is not asserted: torch's fp32
# sums on the CPU depend on the host's vector width and thread count; the bound itself is applied as it comes out.)
FLOAT64_SEEDS = {(64, 32): 2025, (50, 25): 2023, (1024, 512): 2031}


@pytest.mark.gpu
@pytest.mark.parametrize('size', SIZES)
def test_against_float64_on_the_cpu(size):
  """Two frames against torch on the CPU in float64: F.grid_sample over geometry._c2e_grid(..., 'cpu') and the metric formulas
  (tests/panorama_ref.py).  The mean-type metrics, formed in float64 from the device statistics (sum / count, no rounding to fp32),
  must lie within 8 x the distance of the SAME chain in torch CPU fp32 from float64, per frame and per metric; the factor covers
  fp64 sums of fp32 terms against fp32 sums.  A delta_acc count may differ from float64's by at most the number of selected pixels whose
  float64 ratio lies within a relative 1e-4 of the threshold, and that share is at most 0.1 % per threshold.

  The test prints every figure before it asserts.  The same arithmetic evaluated on the host (torch CPU fp32 resampling, fp32 terms,
  fp64 sums) lies 1e-9 .. 4.6e-7 (relative) from float64 for MAE over the three sizes and 1e-9 .. 4.8e-7 for absrel / sqrel, torch CPU
  fp32 itself 3e-9 .. 4.8e-7; RMSE up to 1.6e-6 and silog up to 1.8e-4 at 64 x 32 (the cancellation in mean(l^2) - mean(l)^2) for
  both alike.  The ambiguous share of the delta_acc counts is at most 0.088 % at the three sizes.
  """
  H, W = size
  pred, gt = R.make_inputs(2, H, W, FLOAT64_SEEDS[size])
  ge64 = _assert_gt_clear_of_maxdepth(gt)
  truth, pe64, _ = R.reference_rows(pred, gt, torch.float64)
  ref32, _, _ = R.reference_rows(pred, gt, torch.float32)
  ambiguous = R.ambiguous_counts(pe64, ge64)
  stats = HF.erp_depth_metrics(pred.to(DEV), gt.to(DEV), HG._c2e_grid(W, H, DEV), R.MAXDEPTH, ratio=R.RATIOS).cpu().numpy()
  failures = []
  for f in range(2):
    n_sel, near = ambiguous[f]
    assert stats[f][0] == n_sel == int((ge64[f] <= R.MAXDEPTH).sum())
    ours = R.stat_means(stats[f])
    for k in range(5):
      t = truth[f][k]
      ref_dist, our_dist = abs(ref32[f][k] - t), abs(ours[k] - t)
      print('%dx%d frame %d %-6s float64 %.9g  ours %.3e  torch fp32 %.3e (relative distances)' %
            (H, W, f, R.NAMES[k], t, our_dist / abs(t), ref_dist / abs(t)))
      if not our_dist <= 8 * ref_dist:
        failures.append((f, R.NAMES[k], our_dist, ref_dist))
    for k in range(3):
      assert near[k] <= 1e-3 * n_sel, (f, k, near[k], n_sel)
      count64 = round(truth[f][5 + k] * n_sel / 100)
      got = int(stats[f][mode_hip.M_RATIO + k])
      print('%dx%d frame %d delta%d count %d, float64 %d, ambiguous %d of %d' % (H, W, f, k + 1, got, count64, near[k], n_sel))
      if abs(got - count64) > near[k]:
        failures.append((f, 'delta%d' % (k + 1), got, count64, near[k]))
  assert not failures, failures


@pytest.mark.gpu
def test_selection_edge_cases():
  H, W = 64, 32
  pred, gt = R.make_inputs(3, H, W)
  p, g = pred.to(DEV), gt.to(DEV)
  # a frame with nothing selected: the reference's delta_acc divides by zero on that batch
  far = g.clone()
  far[1] = 5000
  with pytest.raises(ZeroDivisionError, match='frame 1'):
    panorama.erp_depth_metrics(p, far)
  stats = HF.erp_depth_metrics(p, far, HG._c2e_grid(W, H, DEV), R.MAXDEPTH, ratio=R.RATIOS).cpu().numpy()
  assert (stats[1][:9] == 0).all() and stats[0][0] > 0 and stats[2][0] > 0
  # NaN in gt is not selected (every ERP pixel that touches it is NaN, and NaN <= maxdepth is false)
  holes = g.clone()
  holes[0, 30:34, 10:20] = float('nan')
  rows, pe, ge = panorama.erp_depth_metrics(p, holes, return_erp=True)
  assert bool(torch.isnan(ge[0]).any()) and np.isfinite(rows).all()
  s = HF.erp_depth_metrics(p, holes, HG._c2e_grid(W, H, DEV), R.MAXDEPTH, ratio=R.RATIOS).cpu().numpy()
  assert s[0][0] == int((ge[0] <= R.MAXDEPTH).sum()) < int((HG.cassini2Equirec(g[:1].unsqueeze(1))[0] <= R.MAXDEPTH).sum())
  for f in range(3):
    assert rows[f].tobytes() == np.array(E.depth_metrics(pe[f], ge[f], ge[f] <= R.MAXDEPTH)).tobytes()
  # NaN in pred propagates, exactly as in depth_metrics
  bad = p.clone()
  bad[2, 40, 16] = float('nan')
  rows, pe, ge = panorama.erp_depth_metrics(bad, g, return_erp=True)
  assert np.isfinite(rows[:2]).all() and np.isnan(rows[2][:4]).all() and np.isfinite(rows[2][4:]).all()  # (silog takes pred > 0 only)
  ref = np.array(E.depth_metrics(pe[2], ge[2], ge[2] <= R.MAXDEPTH))
  assert np.array_equal(rows[2], ref, equal_nan=True)
  # another maxdepth selects another set
  near_rows = panorama.erp_depth_metrics(p, g, maxdepth=20.)
  assert near_rows.tobytes() == np.array([E.depth_metrics(a, b, b <= 20.) for a, b in zip(*_unfused(p, g)[1:])]).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize('size', [(32, 16), (25, 13), (512, 256)])
@pytest.mark.parametrize('nc', [(2, 1), (1, 3)])
def test_bicubic_up2_against_float64_interpolate(nc, size):
  """The corners are copied exactly; everywhere the distance from torch CPU float64 F.interpolate(scale_factor=[2, 2], mode='bicubic',
  align_corners=True) is at most 4 x the largest deviation of torch CPU fp32 from that float64 on the same input (both are 16-term
  fp32 sums).

  The test prints both figures.  The kernel's arithmetic evaluated on the host (fp32, no fused multiply-adds), inputs in [0, 50):
  max |error| 5.4e-5 / 5.7e-5 / 8.8e-5 at 32 x 16 / 25 x 13 / 512 x 256 against torch CPU fp32's 6.1e-5 / 7.7e-5 / 1.2e-3.
  """
  (N, C), (H, W) = nc, size
  g = torch.Generator().manual_seed(17 + H + C)
  x = torch.rand(N, C, H, W, generator=g) * 50
  y = HF.bicubic_up2(x.to(DEV))
  assert y.shape == (N, C, 2 * H, 2 * W) and y.dtype == torch.float32
  assert panorama.bicubic_up2 is HF.bicubic_up2
  y = y.cpu()
  for a in (0, -1):
    for b in (0, -1):
      assert _bits(y[:, :, a, b]) == _bits(x[:, :, a, b])
  t64 = F.interpolate(x.double(), scale_factor=[2, 2], mode='bicubic', align_corners=True)
  t32 = F.interpolate(x, scale_factor=[2, 2], mode='bicubic', align_corners=True)
  ours, ref = float((y.double() - t64).abs().max()), float((t32.double() - t64).abs().max())
  print('bicubic_up2 (%d,%d) %dx%d: max |error| ours %.3e, torch CPU fp32 %.3e' % (N, C, H, W, ours, ref))
  assert ours <= 4 * ref, (ours, ref)
  assert HF.bicubic_up2(x[:0].to(DEV)).shape == (0, C, 2 * H, 2 * W)


@pytest.mark.gpu
def test_upsampled_scoring_is_the_two_steps():
  """upsample=True: bicubic_up2 of a half-resolution prediction, then the same scoring (test_fusion.py:82, --resize)."""
  H, W = 64, 32
  pred, gt = R.make_inputs(2, H, W)
  half = pred[:, ::2, ::2].contiguous().unsqueeze(1).to(DEV)
  g = gt.to(DEV)
  rows = panorama.erp_depth_metrics(half, g, upsample=True)
  assert _bits(rows) == _bits(panorama.erp_depth_metrics(HF.bicubic_up2(half), g))


@pytest.mark.gpu
def test_graph_replay_is_eager_bit_for_bit():
  from mode_hip.graph_step import GraphedStep
  H, W = 256, 128
  pred, gt = R.make_inputs(3, H, W)
  p, g = pred.to(DEV), gt.to(DEV)
  grid = HG._c2e_grid(W, H, DEV)
  eager = HF.erp_depth_metrics(p, g, grid, R.MAXDEPTH, ratio=R.RATIOS)
  sp, sg = p.clone(), g.clone()
  step = GraphedStep(lambda: HF.erp_depth_metrics(sp, sg, grid, R.MAXDEPTH, ratio=R.RATIOS), static_inputs=(sp, sg))
  for _ in range(2):
    out = step.replay()
    torch.cuda.synchronize()
    assert _bits(out) == _bits(eager)
  p2 = torch.roll(p, 1, 0) * 1.01
  step.load(p2, g)
  out = step.replay()
  torch.cuda.synchronize()
  fresh = HF.erp_depth_metrics(p2, g, grid, R.MAXDEPTH, ratio=R.RATIOS)
  assert _bits(out) == _bits(fresh) and _bits(out) != _bits(eager)


def _tiny_net():
  """The tiny seeded configuration of tests/test_gpu_multiview.py, built afresh: model_wc_tiny's disparity state with its running
  statistics and fusion_tiny's recipe state."""
  z = np.load(os.path.join(recipe.HERE, 'model_wc_tiny.npz'))
  sd = recipe.fixture_state(z)
  for k in z.files:
    if k.startswith('bn/'):
      sd[k[3:]] = torch.from_numpy(z[k]).clone()
  maxdisp, H, W = [int(v) for v in z['cfg'][:3]]
  zf = np.load(os.path.join(recipe.HERE, 'fusion_tiny.npz'))
  cfg = zf['cfg']
  maxdepth, seed, channels = float(cfg[0]), int(cfg[4]), tuple(int(c) for c in cfg[5:])
  manifest = [(k, tuple(s)) for k, s in json.loads(str(zf['manifest']))]
  net = models.ModeMultiView(maxdisp, maxdepth, H, W, channels=channels)
  net.disparity.load_state_dict(sd)
  net.fusion.load_state_dict(recipe.recipe_state(manifest, seed))
  return net.to(DEV).eval(), maxdepth, H, W


@pytest.mark.gpu
def test_multiview_evaluate():
  from mode_hip import no_vendor
  net, maxdepth, H, W = _tiny_net()
  Fr = 2
  left, right = recipe.recipe_images(6 * Fr, H, W, 41)
  frames = torch.stack((left.view(Fr, 6, 3, H, W), right.view(Fr, 6, 3, H, W)), dim=2).reshape(Fr, 12, 3, H, W).to(DEV)
  gen = torch.Generator().manual_seed(43)
  gt = (torch.rand(Fr, H, W, generator=gen) * maxdepth * 1.1).to(DEV)
  depth = net(frames)
  depth_erp, rows = net.evaluate(frames, gt)
  assert depth_erp.shape == (Fr, W, H) and rows.shape == (Fr, 8) and rows.dtype == np.float64
  assert _bits(depth_erp) == _bits(HG.cassini2Equirec(depth))
  with no_vendor.no_vendor_arithmetic() as guard:  # the scoring is our own kernels: no aten interpolation, no grid_sampler
    want = panorama.erp_depth_metrics(depth, gt, maxdepth)
    half = panorama.erp_depth_metrics(depth[:, :, ::2, ::2].contiguous(), gt, maxdepth, upsample=True)
  assert guard.seen > 0
  assert _bits(rows) == _bits(want) and np.isfinite(rows).all() and np.isfinite(half).all()
  sel = HG.cassini2Equirec(gt.unsqueeze(1)) <= maxdepth
  assert 0 < int(sel.sum()) < sel.numel()  # the default maxdepth (the module's own) leaves some ground truth out
  tight = net.evaluate(frames, gt, maxdepth=0.5 * maxdepth)[1]
  assert _bits(tight) == _bits(panorama.erp_depth_metrics(depth, gt, 0.5 * maxdepth)) and _bits(tight) != _bits(rows)
  with pytest.raises(ValueError, match='gt'):
    net.evaluate(frames, gt[:1])
  with pytest.raises(RuntimeError, match='inference only'):
    net.train().evaluate(frames, gt)
