"""The self-supervised stereo loss of DESIGN 22 (HF.photometric_loss, csrc/photometric.hip) restated from its definition as a torch
function on the CPU, in float64 or float32, with autograd into the disparities; and the seeded cases its tests share.

    L, R        = image * std + mean                                  (B, 3, H, W); H is Cassini's periodic axis, W runs pole to pole
    x           = w - d(h, w);  valid iff d finite and 0 <= x <= W - 1
    x0, t       = min(floor(x), W - 2), x - x0;   Rh = (1 - t) R[h, x0] + t R[h, x0 + 1]   (0 where invalid)
    window      the 3x3 neighbourhood of (h, w), 1 <= w <= W - 2, rows modulo H; valid iff its nine pixels are
    ssim        (2 mx my + C1)(2 cxy + C2) / ((mx^2 + my^2 + C1)(vx + vy + C2)) on the centred, biased moments of the window
    pe          mean_c[alpha (1 - ssim_c) / 2 + (1 - alpha) |L_c - Rh_c|(centre)]
    photo_k     sum of pe over the valid windows / max(N_valid_k, 1)
    smooth_k    mean_{w <= W-2} |dn(h, w+1) - dn(h, w)| exp(-beta mean_c |L_c(h, w+1) - L_c(h, w)|) + the same along h (h + 1 modulo H,
                every pixel), dn = d / W
    loss        sum_k wgt[k] (photo_k + lam smooth_k); lam == 0 leaves the smoothness term out altogether (a NaN disparity then costs
                its pixel and nothing else)
"""
import torch

IMAGENET = {'mean': [0.485, 0.456, 0.406], 'std': [0.229, 0.224, 0.225]}
CASES = ((2, 40, 24, 3, 12), (1, 64, 32, 1, 16), (1, 70, 37, 2, 20), (1, 136, 72, 3, 48))  # (B, H, W, K, maxd)
WEIGHTS = (0.5, 0.7, 1.0, 0.9)


def _box(t):
  """Mean over the 3x3 neighbourhood, rows wrapped, for the columns 1 .. W - 2: (..., H, W) -> (..., H, W - 2)."""
  rows = t + torch.roll(t, 1, -2) + torch.roll(t, -1, -2)
  return (rows[..., :-2] + rows[..., 1:-1] + rows[..., 2:]) / 9


def _shifts(t):
  """The nine members of every window, as a leading axis: (..., H, W) -> (9, ..., H, W - 2)."""
  return torch.stack([torch.roll(t, -dy, -2)[..., 1 + dx:t.shape[-1] - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])


def warp(R, d, s=-1):
  """R (B, 3, H, W) de-normalised, d (B, H, W) -> Rh (B, 3, H, W) with zeros at the invalid pixels, valid (B, H, W) bool.  x = w + s d:
  s = -1 is the left view, s = +1 the right view of DESIGN 24."""
  B, _, H, W = R.shape
  w = torch.arange(W, dtype=d.dtype).view(1, 1, W)
  x = w + s * d
  valid = torch.isfinite(d) & (x >= 0) & (x <= W - 1)
  xs = torch.where(valid, x, torch.zeros_like(x))
  x0 = xs.detach().floor().clamp(max=W - 2)
  t = (xs - x0).unsqueeze(1)
  i0 = x0.long().unsqueeze(1).expand(B, 3, H, W)
  Rh = (1 - t) * R.gather(3, i0) + t * R.gather(3, i0 + 1)
  return torch.where(valid.unsqueeze(1), Rh, torch.zeros_like(Rh)), valid


def pe_map(L, Rh, valid, alpha, C1=1e-4, C2=9e-4):
  """The window term between L and a warped image Rh (B, 3, H, W) with its validity (B, H, W): -> (pe, wvalid), both (B, H, W - 2)."""
  wvalid = _shifts(valid).all(0)
  mx, my = _box(L), _box(Rh)
  xs, ys = _shifts(L) - mx, _shifts(Rh) - my
  vx, vy, cxy = (xs * xs).mean(0), (ys * ys).mean(0), (xs * ys).mean(0)
  ssim = (2 * mx * my + C1) * (2 * cxy + C2) / ((mx * mx + my * my + C1) * (vx + vy + C2))
  l1 = (L - Rh).abs()[..., 1:-1]
  return (alpha * (1 - ssim) / 2 + (1 - alpha) * l1).mean(1), wvalid


def loss_terms(left, right, d, alpha=0.85, beta=1.0, C1=1e-4, C2=9e-4, mean=None, std=None, s=-1, mask=None):
  """One disparity map d (B, H, W) -> (N_valid (python int), photo, smooth) in d's dtype.  s, mask: `left` is the view's own
  image, x = w + s d, and a mask (B, H, W) is and-ed into the validity of a pixel."""
  dt = d.dtype
  mean = torch.tensor(IMAGENET['mean'] if mean is None else mean, dtype=dt).view(1, 3, 1, 1)
  std = torch.tensor(IMAGENET['std'] if std is None else std, dtype=dt).view(1, 3, 1, 1)
  L, R = left.to(dt) * std + mean, right.to(dt) * std + mean
  B, _, H, W = L.shape
  Rh, valid = warp(R, d, s)
  if mask is not None:
    valid = valid & (mask != 0)
  pe, wvalid = pe_map(L, Rh, valid, alpha, C1, C2)
  n = int(wvalid.sum())
  photo = torch.where(wvalid, pe, torch.zeros_like(pe)).sum() / max(n, 1)
  dn = d / W
  ex = torch.exp(-beta * (L[..., 1:] - L[..., :-1]).abs().mean(1))
  ey = torch.exp(-beta * (torch.roll(L, -1, -2) - L).abs().mean(1))
  smooth = ((dn[..., 1:] - dn[..., :-1]).abs() * ex).mean() + ((torch.roll(dn, -1, -2) - dn).abs() * ey).mean()
  return n, photo, smooth


def photometric_loss(left, right, disps, weights, alpha=0.85, lam=0.1, beta=1.0, mean=None, std=None, s=-1, masks=None):
  """disps: K tensors (B, H, W); masks: None or (K, B, H, W) -> (loss, stats (K, 3) = [N_valid, photo, smooth] detached)."""
  loss, rows = 0, []
  for k, (d, wgt) in enumerate(zip(disps, weights)):
    n, photo, smooth = loss_terms(left, right, d, alpha, beta, mean=mean, std=std, s=s, mask=None if masks is None else masks[k])
    loss = loss + wgt * (photo + lam * smooth if lam != 0 else photo)
    rows.append(torch.stack([torch.tensor(float(n), dtype=d.dtype), photo.detach(), smooth.detach()]))
  return loss, torch.stack(rows)


def brute_force_count(left, right, d):
  """N_valid of one map by loops over the definition (float64 x)."""
  B, H, W = d.shape
  dd = d.double()
  ok = [[[bool(torch.isfinite(dd[b, h, w])) and 0 <= w - float(dd[b, h, w]) <= W - 1 for w in range(W)] for h in range(H)] for b in range(B)]
  n = 0
  for b in range(B):
    for h in range(H):
      for w in range(1, W - 1):
        n += all(ok[b][(h + dy) % H][w + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
  return n


def _lowpass(u):
  """Uniform noise averaged with its left and upper neighbours (rows wrapped, the first column kept)."""
  left = torch.cat([u[..., :1], u[..., :-1]], -1)
  return (u + left + torch.roll(u, 1, -2)) / 3


def make_case(B, H, W, K, maxd, seed=0):
  """Seeded float32 inputs: left, right (B, 3, H, W) normalised, disps: K maps (B, H, W).  The right image is half independent noise;
  disp = floor(U maxd) - 2 + 0.05 + 0.9 U', so that the fractional part of w - d stays in [0.05, 0.95], away from the kink of floor;
  some disparities are negative and some push x below 0."""
  g = torch.Generator().manual_seed(1000 * seed + 7 * H + W)
  mean = torch.tensor(IMAGENET['mean']).view(1, 3, 1, 1)
  std = torch.tensor(IMAGENET['std']).view(1, 3, 1, 1)
  base = _lowpass(torch.rand(B, 3, H, W, generator=g, dtype=torch.float64))
  other = _lowpass(torch.rand(B, 3, H, W, generator=g, dtype=torch.float64))
  left = ((base - mean) / std).float()
  right = ((0.5 * base + 0.5 * other - mean) / std).float()
  disps = []
  for _ in range(K):
    u, u2 = torch.rand(B, H, W, generator=g, dtype=torch.float64), torch.rand(B, H, W, generator=g, dtype=torch.float64)
    disps.append((torch.floor(u * maxd) - 2 + 0.05 + 0.9 * u2).float())
  return left, right, disps


_cache = {}


def reference(case, dtype, **kw):
  """(loss, stats, [gdisp_k]) of a case in `dtype` on the CPU, computed once per (case, dtype, parameters) and shared."""
  key = (case, dtype, tuple(sorted(kw.items())))
  if key not in _cache:
    left, right, disps = make_case(*case)
    ds = [d.to(dtype).requires_grad_(True) for d in disps]
    loss, stats = photometric_loss(left, right, ds, WEIGHTS[:len(ds)], **kw)
    grads = torch.autograd.grad(loss, ds, allow_unused=True)
    grads = [torch.zeros_like(d) if g is None else g for g, d in zip(grads, ds)]
    _cache[key] = (loss.detach(), stats, grads)
  return _cache[key]


def yardstick(got32, want64):
  """The float32 restatement's own error of a quantity against float64, relative to max|want64| and never below one fp32 ulp of it
  (a correctly rounded fp32 result already errs by half an ulp: a smaller yardstick is luck; DESIGN 24's bound).  -> (yardstick, scale)."""
  want64 = torch.as_tensor(want64, dtype=torch.float64)
  scale = float(want64.abs().max())
  if scale == 0:
    return 0.0, 0.0
  err = float((torch.as_tensor(got32).double() - want64).abs().max()) / scale
  return max(err, 2.0 ** -23), scale


def error(got, want64, scale):
  want64 = torch.as_tensor(want64, dtype=torch.float64)
  diff = float((torch.as_tensor(got).double() - want64).abs().max())
  return diff / scale if scale else diff
