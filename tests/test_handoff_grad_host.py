"""The gradient of the multi-view hand-off, CPU tier: the adjoint lists of the rotation grids, the float64 oracle (tests/handoff_ref.py)
against numerical differentiation, the host-side argument checks of mode_multiview_handoff_bwd (no launch) and the module contract of
ModeMultiView.fusion_loss."""
import ctypes
import math

import numpy as np
import pytest
import torch

import handoff_ref as R
import mode_hip
import models
from utils import geometry as HG


def _taps64(grid, H, W):
  """The bilinear taps of an (H, W, 2) float32 grid in float64 as a dense (targets, sources) matrix, and per target the number of
  corners inside the image as float32 arithmetic places them."""
  A = np.zeros((H * W, H * W))
  inside = np.zeros(H * W, dtype=np.int64)
  g = grid.reshape(H * W, 2)
  for t in range(H * W):
    x = min(max((float(g[t, 0]) + 1.0) * 0.5 * (W - 1), 0.0), W - 1.0)
    y = min(max((float(g[t, 1]) + 1.0) * 0.5 * (H - 1), 0.0), H - 1.0)
    x0, y0 = int(math.floor(x)), int(math.floor(y))
    wx1, wy1 = x - x0, y - y0
    for yy, xx, w in ((y0, x0, (1 - wx1) * (1 - wy1)), (y0, x0 + 1, wx1 * (1 - wy1)), (y0 + 1, x0, (1 - wx1) * wy1), (y0 + 1, x0 + 1, wx1 * wy1)):
      if xx <= W - 1 and yy <= H - 1:
        A[t, yy * W + xx] += w
    x32 = np.float32(min(max((g[t, 0] + np.float32(1)) * np.float32(0.5) * np.float32(W - 1), np.float32(0)), np.float32(W - 1)))
    y32 = np.float32(min(max((g[t, 1] + np.float32(1)) * np.float32(0.5) * np.float32(H - 1), np.float32(0)), np.float32(H - 1)))
    x1ok, y1ok = int(np.floor(x32)) + 1 <= W - 1, int(np.floor(y32)) + 1 <= H - 1
    inside[t] = 1 + x1ok + y1ok + (x1ok and y1ok)
  return A, inside


@pytest.mark.parametrize('size', [(64, 32), (48, 24)])
def test_adjoint_lists_are_the_transposed_taps(size):
  H, W = size
  hw = H * W
  HG._adjoint_cache.clear()
  rowptr, target, weight = HG._frames_adjoint(H, W, 'cpu')
  assert HG._frames_adjoint(H, W, 'cpu')[0] is rowptr  # cached
  assert rowptr.dtype == torch.int32 and target.dtype == torch.int32 and weight.dtype == torch.float32
  assert tuple(rowptr.shape) == (2, hw + 1) and target.shape == weight.shape == (int(rowptr[1, hw]),)
  rp, tg, wt = rowptr.numpy().astype(np.int64), target.numpy().astype(np.int64), weight.numpy()
  assert rp[0, 0] == 0 and rp[1, 0] == rp[0, hw] and (np.diff(rp.ravel()) >= 0).all()
  assert len(tg) <= 8 * hw and tg.min() >= 0 and tg.max() < hw and (wt >= 0).all() and (wt <= 1).all()
  for g, pair in enumerate(('13', '14')):
    A64, inside = _taps64(R.rot_grid(H, W, pair)[0].numpy(), H, W)
    lo, hi = rp[g, 0], rp[g, hw]
    src = np.repeat(np.arange(hw), np.diff(rp[g]))
    t, w = tg[lo:hi], wt[lo:hi]
    assert len(src) == hi - lo
    # sorted by source, then target; a corner of a tap is one source, so a (source, target) pair appears once
    order = src * hw + t
    assert (np.diff(order) > 0).all()
    assert np.array_equal(np.bincount(t, minlength=hw), inside)  # every corner inside the image, exactly once
    A = np.zeros((hw, hw))
    A[t, src] = w
    # float32 rounding: the sample coordinate is below max(H, W), a few ulp of it reach every weight
    tol = 8 * 2.0 ** -24 * max(H, W)
    assert np.abs(A - A64).max() <= tol, (pair, np.abs(A - A64).max(), tol)
    assert np.abs(A.sum(1) - 1).max() <= tol  # border padding: the taps of a target sum to 1


def _smooth_case(seed=3):
  """An 8 x 4 map whose disparities keep every pixel strictly inside the sine rule's range (0 < raw < 1000, far from both clips),
  with fixed winners: some targets empty, some sources winning."""
  F_, H, W = 1, 8, 4
  g = torch.Generator().manual_seed(seed)
  disp = 0.2 + 0.2 * torch.rand(F_, 6, H, W, generator=g, dtype=torch.float64)
  winners = torch.randint(0, H * W, (F_, 3, H, W), generator=g)
  winners[torch.rand(F_, 3, H, W, generator=g) < 0.2] = -1
  return disp, winners


@pytest.mark.parametrize('dbname', ['Deep360', 'other'])
def test_oracle_against_numerical_differentiation(dbname):
  disp, winners = _smooth_case()
  for p in range(6):
    raw = R.sine_rule_raw(disp[:, p], HG._baselines(dbname)[p], torch.float64)
    assert float(raw.min()) > 0.05 and float(raw.max()) < 100 and not bool(R.near_kink(disp[:, p], HG._baselines(dbname)[p]).any())
  d = disp.clone().requires_grad_(True)
  assert torch.autograd.gradcheck(lambda x: R.handoff_depth(x, winners, dbname, torch.float64), (d,), eps=1e-6, atol=1e-6, rtol=1e-6)
  # the closed form of the sine rule's slope is what autograd finds
  for p in range(6):
    b = HG._baselines(dbname)[p]
    x = disp[:, p].clone().requires_grad_(True)
    g, = torch.autograd.grad(R.sine_rule(x, b, torch.float64).sum(), x)
    s = R.slope(disp[:, p], b)
    assert float((g - s).abs().max()) <= 1e-12 * float(s.abs().max())


def test_oracle_structural_zeros():
  """d == 0 and both clips give a zero gradient in the oracle, the clip boundaries' own side passes."""
  disp = torch.tensor([[0.0, 1e-4, 0.3, 3.9]], dtype=torch.float64).expand(8, 4).contiguous()
  s = R.slope(disp, 1.0)
  assert bool((s[:, 0] == 0).all()) and bool((s[:, 1] == 0).all()) and bool((s[:, 2] < 0).all())
  raw = R.sine_rule_raw(disp, 1.0, torch.float64)
  assert bool((raw[:, 1] > 1000).all()) and bool((raw[:, 3] < 0).all()) and bool((s[:, 3] == 0).all())
  x = disp.clone().requires_grad_(True)
  g, = torch.autograd.grad(R.sine_rule(x, 1.0, torch.float64).sum(), x)
  assert torch.equal(g == 0, s == 0) and float((g - s).abs().max()) <= 1e-12 * float(s.abs().max())


def test_key_decoding():
  H, W = 4, 2
  bits = lambda v: int(np.float32(v).view(np.uint32))
  keys = torch.tensor([-1, (bits(2.5) << 32) | (1 << 31) | 5, (bits(7.0) << 32) | (H * W - 1 - 3), (bits(1200.0) << 32) | (1 << 31)] + [-1] * 4,
                      dtype=torch.int64).view(H, W)
  winner, v = R.decode_keys(keys)
  assert winner.view(-1)[:4].tolist() == [-1, 5, 3, 0] and v.view(-1)[:4].tolist() == [0.0, 2.5, 7.0, 1200.0]


def test_backward_entry_validates_on_the_host():
  lib = mode_hip.lib()
  null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
  b6 = (ctypes.c_float * 6)(*[1.0] * 6)
  xf = (ctypes.c_double * 36)()

  def call(F=1, H=64, W=32, disp=one, gout=one, keys=one, base=ctypes.cast(b6, ctypes.c_void_p), trig=one, x=ctypes.cast(xf, ctypes.c_void_p),
           rowptr=one, target=one, weight=one, n=16, flags=0, gdisp=one):
    return lib.mode_multiview_handoff_bwd(disp, gout, keys, F, H, W, base, trig, x, rowptr, target, weight, n, flags, gdisp, null)

  assert call(F=-1) == -1 and b'bad size' in lib.mode_last_error()
  assert call(H=0) == -1 and call(W=-4) == -1
  assert call(F=1 << 10, H=1024, W=1024) == -1 and b'bad size' in lib.mode_last_error()  # 3 F H W >= 2^31
  assert call(flags=4) == -1 and b'flags' in lib.mode_last_error()
  assert call(n=-1) == -1 and b'adjoint' in lib.mode_last_error()
  assert call(n=8 * 64 * 32 + 1) == -1 and b'adjoint' in lib.mode_last_error()
  for kw in ('disp', 'gout', 'base', 'trig', 'x', 'rowptr', 'target', 'weight', 'gdisp'):
    assert call(**{kw: null}) == -1 and b'null pointer' in lib.mode_last_error(), kw
  assert call(keys=null) == -3 and b'key planes' in lib.mode_last_error()
  assert call(keys=ctypes.c_void_p(20)) == -3 and b'unaligned' in lib.mode_last_error()
  assert call(F=0, disp=null, gout=null, keys=null, gdisp=null) == 0  # nothing to do
  assert 'mode_multiview_handoff_bwd' in mode_hip.SIGNATURES


def test_cpu_tensors_and_wrong_modes_are_refused():
  net = models.ModeMultiView(16, 10., 64, 32, channels=(8, 16, 32, 64))
  frames, gt = torch.zeros(1, 12, 3, 64, 32), torch.ones(1, 64, 32)
  with pytest.raises(NotImplementedError):
    net.train().fusion_loss(frames, gt)
  net.disparity.eval()
  with pytest.raises(NotImplementedError):
    net.fusion_loss(frames, gt)
  net.fusion.eval()
  with pytest.raises(RuntimeError, match='fusion_loss'):
    net.fusion_loss(frames, gt)
  with pytest.raises(RuntimeError, match='inference only'):
    net.train()(frames)
  half = models.ModeMultiView(16, 10., 64, 32, channels=(8, 16, 32, 64), resize=True).train()
  with pytest.raises(ValueError, match='no backward'):
    half.fusion_loss(torch.zeros(1, 12, 64, 32, 3, dtype=torch.uint8), gt)
  with pytest.raises(NotImplementedError):
    HG.disp2depth_frames_gpu(torch.zeros(1, 6, 64, 32, requires_grad=True), torch.zeros(1, 6, 64, 32), return_keys=True)
  with pytest.raises(NotImplementedError):
    HG.disp2depth_frames_bwd(torch.zeros(1, 6, 64, 32), torch.zeros(1, 12, 64, 32), torch.zeros(1, 3, 64, 32, dtype=torch.int64))
