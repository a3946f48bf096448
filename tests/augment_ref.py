"""Host restatement of the colour augmentation (tests/test_augment_host.py, tests/test_gpu_augment.py,
tests/test_gpu_guard_bands_augment.py): the transform of include/mode_hip.h's mode_images_u8_augment block -- the reference's
inception_color_preproccess (dataloader/preprocess.py:33-46, 78-95) with torchvision's tensor path written out -- in torch on the CPU,
one tensor operation per rounding, in float32 or (the same code on .double() inputs) in float64.  Nothing here touches the GPU.

float64 runs start from the SAME float32 constants and coefficients (widened), so the difference between the two runs is the
float32 rounding of the arithmetic alone: that is E_ref, the reference's own error, which the GPU test's bound is made of."""
import functools

import numpy as np
import torch

import ingest_ref as R

GREY = (0.2989, 0.587, 0.114)
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
BRIGHTNESS, CONTRAST, SATURATION, NONE = 0, 1, 2, -1

ORDERS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
ROWS = ORDERS + [(NONE, NONE, NONE), (SATURATION, NONE, NONE)]  # the N = 8 images of a case: six orders, nothing, saturation alone
FACTOR_SETS = [(0.6, 0.6, 0.6), (1.4, 1.4, 1.4), (0.6, 1.4, 0.83), (1.25, 0.7, 1.4)]  # (brightness, contrast, saturation)
SIZES = [(8, 12), (48, 32), (96, 80)]  # 24 quads: less than a block; 384: one and a half; 1 920: several blocks, ragged last one


def _c(values, dtype):
  """float32 constants, widened to dtype: (3, 1, 1)."""
  return torch.tensor(values, dtype=torch.float32).to(dtype).view(3, 1, 1)


def grey(x):
  k = _c(GREY, x.dtype)
  return (k[0] * x[0] + k[1] * x[1]) + k[2] * x[2]


def blend(a, b, rho, sigma):
  return (rho * a + sigma * b).clamp(0, 1)


def augment(image_u8, ops, coef, dtype=torch.float32, mean=None):
  """One (H, W, 3) uint8 image, its row of operation codes (3) and of coefficients (9 float32: rho, sigma of brightness, contrast,
  saturation; three shifts) -> (out (3, H, W) of dtype, info).  mean: use this contrast mean (a float32 value, e.g. the kernel's own)
  instead of torch.mean.  info: 'mean' the contrast mean used (None without a contrast step), 'grey_mean64' the float64 mean of the
  grey image of THIS run at the contrast step."""
  coef = torch.as_tensor(coef, dtype=torch.float32).to(dtype)
  x = torch.from_numpy(np.ascontiguousarray(np.asarray(image_u8).transpose(2, 0, 1))).to(torch.float32).div(255).to(dtype)
  info = {'mean': None, 'grey_mean64': None}
  seen = set()
  for op in [int(o) for o in ops]:
    if op not in (BRIGHTNESS, CONTRAST, SATURATION):
      continue
    assert op not in seen, 'an operation appears at most once'
    seen.add(op)
    rho, sigma = coef[2 * op], coef[2 * op + 1]
    if op == BRIGHTNESS:
      x = blend(x, torch.zeros_like(x), rho, sigma)
    elif op == CONTRAST:
      g = grey(x)
      info['grey_mean64'] = float(g.double().mean())
      m = g.mean() if mean is None else torch.as_tensor(mean, dtype=torch.float32).to(dtype)
      info['mean'] = m.clone()
      x = blend(x, m, rho, sigma)
    else:
      x = blend(x, grey(x).unsqueeze(0), rho, sigma)
  x = x + coef[6:9].view(3, 1, 1)
  return (x - _c(MEAN, dtype)) / _c(STD, dtype), info


def augment_batch(images_u8, ops, coef, dtype=torch.float32, means=None):
  """(N, H, W, 3) uint8 -> (out (N, 3, H, W), [info])."""
  outs, infos = [], []
  for n in range(len(images_u8)):
    o, i = augment(images_u8[n], ops[n], coef[n], dtype, None if means is None else means[n])
    outs.append(o)
    infos.append(i)
  return torch.stack(outs), infos


def tables(rows, factors, shifts):
  """Host tables as dataloader.gpu_ingest.ColourParams lays them out, built here independently: ops (n, 3) int32, coef (n, 9) float32."""
  n = len(rows)
  ops = np.full((n, 3), NONE, dtype=np.int32)
  coef = np.zeros((n, 9), dtype=np.float32)
  for i, row in enumerate(rows):
    ops[i, :len(row)] = row
    for k in range(3):
      f = float(factors[i][k])
      coef[i, 2 * k] = np.float32(f)
      coef[i, 2 * k + 1] = np.float32(1.0 - f)  # in double, then rounded: torch's (1.0 - ratio) * img with a Python scalar
    coef[i, 6:] = shifts[i]
  return ops, coef


def case_shifts(n, seed):
  """n lighting shifts from seeded alphas of standard deviation 0.1, through the product's own lighting_shift (pinned to the
  reference by tests/golden/augment_lighting.npz)."""
  from dataloader import gpu_ingest
  alphas = torch.from_numpy((0.1 * np.random.RandomState(seed).standard_normal((n, 3))).astype(np.float32))
  return torch.stack([gpu_ingest.lighting_shift(a) for a in alphas]).numpy()


def case(H, W, factors, kind='random'):
  """The GPU test's case at one size and one factor set: 8 images of tests/ingest_ref.py, ROWS, per-image shifts -> (images (8, H, W, 3)
  uint8, rows, factor rows (8, 3), shifts (8, 3))."""
  images = R.frames_u8(1, H, W, 700 + H, kind)[0, :len(ROWS)]
  return images, list(ROWS), [tuple(factors)] * len(ROWS), case_shifts(len(ROWS), 800 + W)


@functools.lru_cache(maxsize=None)
def e_ref():
  """max |float32 restatement - float64 restatement| of the normalised output over the GPU test's case set."""
  worst = 0.0
  for H, W in SIZES:
    for factors in FACTOR_SETS:
      images, rows, frows, shifts = case(H, W, factors)
      ops, coef = tables(rows, frows, shifts)
      a, _ = augment_batch(images, ops, coef, torch.float32)
      b, _ = augment_batch(images, ops, coef, torch.float64)
      worst = max(worst, float((a.double() - b).abs().max()))
  return worst
