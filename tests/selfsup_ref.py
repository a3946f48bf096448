"""The bidirectional self-supervised loss of DESIGN 24 (HF.lr_consistency, HF.photometric_loss(view=, masks=); csrc/lr_consistency.hip,
csrc/photometric.hip) restated from its definition as torch functions on the CPU, in float64 or float32, with autograd into the
disparities; and the seeded cases its tests share.

A view is (s, own, other): left = (-1, dl, dr), right = (+1, dr, dl).

    x        = w + s own(h, w)
    valid    iff own finite, 0 <= own <= dmax, 0 <= x <= W - 1, and other[h, x0], other[h, x0 + 1] both finite
    x0, t    = min(floor(x), W - 2), x - x0;   oh = (1 - t) other[h, x0] + t other[h, x0 + 1]
    e        = |own - oh|  (0 where invalid);  vis = valid and e <= tau
    lr_v_k   = sum of e over valid pixels / max(N_valid, 1);   loss = sum_k wgt[k] (lr_left_k + lr_right_k)

The view loss is tests/photometric_ref.py's with x = w + s d and an optional mask that is and-ed into the validity of a pixel.
"""
import torch

import photometric_ref as R

CASES = R.CASES  # (B, H, W, K, maxd); tau = maxd / 4, dmax = maxd
WEIGHTS = R.WEIGHTS
VIEWS = ((-1, 0, 1), (1, 1, 0))  # (s, index of own, index of other) in (dl, dr)


def lr_view(own, other, s, tau, dmax):
  """own, other (B, H, W) -> (e with zeros at the invalid pixels, valid, vis)."""
  W = own.shape[-1]
  zero = torch.zeros_like(own)
  w = torch.arange(W, dtype=own.dtype).view(1, 1, W)
  x = w + s * own
  valid = torch.isfinite(own) & (own >= 0) & (own <= dmax) & (x >= 0) & (x <= W - 1)
  own_s = torch.where(valid, own, zero)  # (no NaN reaches the arithmetic: 0 x NaN would spoil the gradient)
  xs = torch.where(valid, w + s * own_s, zero)
  x0 = xs.detach().floor().clamp(max=W - 2)
  t = xs - x0
  i0 = x0.long()
  o0, o1 = other.gather(2, i0), other.gather(2, i0 + 1)
  valid = valid & torch.isfinite(o0) & torch.isfinite(o1)
  o0, o1 = torch.where(valid, o0, zero), torch.where(valid, o1, zero)
  e = torch.where(valid, (own_s - ((1 - t) * o0 + t * o1)).abs(), zero)
  return e, valid, valid & (e.detach() <= tau)


def lr_consistency(dls, drs, weights, tau, dmax):
  """K maps (B, H, W) per view -> (loss, stats (2, K, 3) = [N_valid, lr, N_visible] detached, masks (2, K, B, H, W) bool)."""
  loss, rows, masks = 0, [[], []], [[], []]
  for dl, dr, wgt in zip(dls, drs, weights):
    pair = (dl, dr)
    for v, (s, own, other) in enumerate(VIEWS):
      e, valid, vis = lr_view(pair[own], pair[other], s, tau, dmax)
      n = int(valid.sum())
      lr = e.sum() / max(n, 1)
      loss = loss + wgt * lr
      rows[v].append(torch.stack([torch.tensor(float(n), dtype=dl.dtype), lr.detach(), torch.tensor(float(int(vis.sum())), dtype=dl.dtype)]))
      masks[v].append(vis)
  return loss, torch.stack([torch.stack(r) for r in rows]), torch.stack([torch.stack(m) for m in masks])


warp = R.warp  # (Rimg, d, s): photometric_ref.warp with x = w + s d


def view_terms(own_image, other_image, d, s, mask=None, alpha=0.85, beta=1.0, C1=1e-4, C2=9e-4):
  """photometric_ref.loss_terms from either camera: one map d (B, H, W) -> (N_valid, photo, smooth)."""
  return R.loss_terms(own_image, other_image, d, alpha, beta, C1, C2, s=s, mask=mask)


def view_loss(own_image, other_image, disps, weights, s, masks=None, alpha=0.85, lam=0.1, beta=1.0):
  """disps: K tensors (B, H, W); masks: None or (K, B, H, W) -> (loss, stats (K, 3) = [N_valid, photo, smooth] detached)."""
  return R.photometric_loss(own_image, other_image, disps, weights, alpha, lam, beta, s=s, masks=masks)


def make_case(B, H, W, K, maxd):
  """Seeded float32 inputs: the images of photometric_ref.make_case and K left and K right maps (B, H, W), drawn as
  floor(U maxd) - 1 + 0.05 + 0.9 U': the fractional part of w -/+ d stays in [0.05, 0.95], and a few maps' values are negative."""
  left, right, _ = R.make_case(B, H, W, K, maxd)
  g = torch.Generator().manual_seed(7 * H + W + 1)
  dls, drs = [], []
  for maps in (dls, drs):
    for _ in range(K):
      u, u2 = torch.rand(B, H, W, generator=g, dtype=torch.float64), torch.rand(B, H, W, generator=g, dtype=torch.float64)
      maps.append((torch.floor(u * maxd) - 1 + 0.05 + 0.9 * u2).float())
  return left, right, dls, drs


def block_mask(B, H, W, K, maxd):
  """(K, B, H, W) bool: about a quarter of the 5 x 7 blocks zero.  The consistency masks of make_case's independent maps leave hardly
  a window of nine visible pixels; this one leaves most of them, with edges on every side of the holes."""
  g = torch.Generator().manual_seed(7 * H + W + 2)
  hb, wb = -(-H // 5), -(-W // 7)
  keep = torch.rand(K, B, hb, wb, generator=g) >= 0.25
  return keep.repeat_interleave(5, 2).repeat_interleave(7, 3)[:, :, :H, :W].contiguous()


def params(case):
  """(tau, dmax) of a case."""
  return case[4] / 4.0, float(case[4])


_cache = {}


def _grads(loss, xs):
  got = torch.autograd.grad(loss, xs, allow_unused=True)
  return [torch.zeros_like(x) if g is None else g for g, x in zip(got, xs)]


def lr_reference(case, dtype):
  """(loss, stats (2, K, 3), masks (2, K, B, H, W) bool, [gdl_k], [gdr_k]) in `dtype`, computed once per (case, dtype) and shared."""
  key = ('lr', case, dtype)
  if key not in _cache:
    _, _, dls, drs = make_case(*case)
    K = len(dls)
    tau, dmax = params(case)
    xs = [d.clone().to(dtype).requires_grad_(True) for d in dls + drs]
    loss, stats, masks = lr_consistency(xs[:K], xs[K:], WEIGHTS[:K], tau, dmax)
    g = _grads(loss, xs)
    _cache[key] = (loss.detach(), stats, masks, g[:K], g[K:])
  return _cache[key]


def view_reference(case, dtype, view, masked):
  """(loss, stats (K, 3), [gdisp_k]) of the view loss of a case: view 0 on (left, right, dl), view 1 on (right, left, dr); masked: False, True
  (the float64 consistency masks of that view) or 'blocks' (block_mask)."""
  key = ('view', case, dtype, view, masked)
  if key not in _cache:
    left, right, dls, drs = make_case(*case)
    own, other, maps = (left, right, dls) if view == 0 else (right, left, drs)
    masks = None
    if masked == 'blocks':
      masks = block_mask(*case)
    elif masked:
      masks = lr_reference(case, torch.float64)[2][view]
    xs = [d.clone().to(dtype).requires_grad_(True) for d in maps]
    loss, stats = view_loss(own, other, xs, WEIGHTS[:len(xs)], VIEWS[view][0], masks)
    _cache[key] = (loss.detach(), stats, _grads(loss, xs))
  return _cache[key]


yardstick, error = R.yardstick, R.error  # the bound of the GPU tests: the float32 restatement's own error against float64


def two_planes():
  """H = 8, W = 40: a background of disparity 4 and a strip of disparity 9 on the left view's columns 20..27, which the right camera sees
  on its columns 11..18.  -> (dl, dr) (1, H, W) float64."""
  dl, dr = torch.full((1, 8, 40), 4.0, dtype=torch.float64), torch.full((1, 8, 40), 4.0, dtype=torch.float64)
  dl[..., 20:28] = 9.0
  dr[..., 11:19] = 9.0
  return dl, dr
