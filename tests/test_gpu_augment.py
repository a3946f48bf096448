"""GPU tier of the colour augmentation (csrc/augment.hip) against the host restatement of tests/augment_ref.py.

The rules, from the contract in include/mode_hip.h:
  * without a contrast step the output is the float32 restatement's, bit for bit;
  * with one, the returned mean lies within 2^-24 of the float64 mean of the restatement's grey image at that step (values in [0, 1],
    one float32 rounding, an fp64 accumulation error below H W 2^-53), the output equals bit for bit the float32 restatement FED that
    mean, and it lies within 4 E_ref of the float64 restatement -- E_ref the float32 restatement's own distance from it over this
    file's case set (tests/augment_ref.e_ref), the factor 4 for the two differently ordered mean sums on top of it.
The images are those of tests/ingest_ref.py: every byte value in every channel, and the 0 / 255 kind for the clamps."""
import numpy as np
import pytest
import torch

import augment_ref as A
import ingest_ref as R

from dataloader import gpu_ingest as G
from mode_hip import functional as HF

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _params(rows, factors, shifts):
  return G.ColourParams(rows, factors, None if shifts is None else torch.from_numpy(np.asarray(shifts, dtype=np.float32)), DEV)


def _check(images, rows, factors, shifts, out, means, e_ref=None):
  """The rules above for one batch; out (N, 3, H, W) and means (N,) on the host."""
  ops, coef = A.tables(rows, factors, shifts)
  fed, infos = A.augment_batch(images, ops, coef, torch.float32, means=means)
  plain, _ = A.augment_batch(images, ops, coef, torch.float32)
  exact = A.augment_batch(images, ops, coef, torch.float64)[0] if e_ref is not None else None
  worst_mean = worst = 0.0
  for n in range(len(images)):
    if infos[n]['mean'] is None:
      assert float(means[n]) == 0 and torch.equal(out[n], plain[n]), 'image %d (no contrast step) differs from the restatement' % n
    else:
      d = abs(float(means[n]) - infos[n]['grey_mean64'])
      worst_mean = max(worst_mean, d)
      assert d <= 2.0 ** -24, 'image %d: mean off by %.3e' % (n, d)
      assert torch.equal(out[n], fed[n]), 'image %d differs from the restatement fed the returned mean' % n
    if exact is not None:
      worst = max(worst, float((out[n].double() - exact[n]).abs().max()))
  print('  worst mean distance %.3e (bound %.3e)' % (worst_mean, 2.0 ** -24))
  if exact is not None:
    print('  worst distance from float64 %.3e (bound 4 E_ref = %.3e)' % (worst, 4 * e_ref))
    assert worst <= 4 * e_ref


@pytest.mark.parametrize('H,W', A.SIZES)
def test_orders_and_factors_against_the_restatement(H, W):
  e_ref = A.e_ref()
  for factors in A.FACTOR_SETS:
    images, rows, frows, shifts = A.case(H, W, factors)
    p = _params(rows, frows, shifts)
    ops, coef = A.tables(rows, frows, shifts)
    assert np.array_equal(p.ops_host.numpy(), ops) and np.array_equal(p.coef_host.numpy(), coef)  # two independent table builders
    out, means = G.augment_u8_gpu(torch.from_numpy(images).to(DEV), p, return_means=True)
    assert tuple(out.shape) == (len(rows), 3, H, W) and out.dtype == torch.float32
    _check(images, rows, frows, shifts, out.cpu(), means.cpu(), e_ref)


@pytest.mark.parametrize('factors', [(0.0, 0.0, 0.0), (2.0, 2.0, 2.0), (0.0, 2.0, 0.0), (2.0, 0.0, 2.0)])
def test_extreme_factors_on_binary_images(factors):
  """Factors 0 and 2 on 0 / 255 images: both clamp ends (2 x 1 > 1; contrast 2 on a dark pixel < 0) and, with saturation 0, a grey-only
  image."""
  H, W = 48, 32
  images, rows, frows, shifts = A.case(H, W, factors, 'binary')
  shifts = np.zeros_like(shifts)
  out, means = G.augment_u8_gpu(torch.from_numpy(images).to(DEV), _params(rows, frows, shifts), return_means=True)
  out, means = out.cpu(), means.cpu()
  _check(images, rows, frows, shifts, out, means)  # (the bit-for-bit rules; E_ref is not measured at these factors)
  x = out *torch.tensor(A.STD).view(1, 3, 1, 1) + torch.tensor(A.MEAN).view(1, 3, 1, 1)  # un-normalised, to 1e-6
  n_ops = [n for n, r in enumerate(rows) if any(c >= 0 for c in r)]
  assert float(x[n_ops].min()) > -1e-6 and float(x[n_ops].max()) < 1 + 1e-6  # the operations clamp
  if factors[2] == 0.0:
    sat_last = [n for n, r in enumerate(rows) if tuple(r)[-1] == A.SATURATION]
    assert sat_last and all(float((x[n, 0] - x[n, 1]).abs().max()) < 1e-6 and float((x[n, 1] - x[n, 2]).abs().max()) < 1e-6 for n in sat_last)


def test_identity_is_the_plain_ingest():
  F, H, W = 2, 48, 32
  frames = torch.from_numpy(R.frames_u8(F, H, W, 41)).to(DEV)
  p = _params([()] * (12 * F), [(1, 1, 1)] * (12 * F), None)
  want = G.frames_u8_gpu(frames)
  got = G.frames_u8_gpu(frames, augment=p)
  for a, b in zip(got, want):
    assert a.shape == b.shape and a.is_contiguous() and torch.equal(a, b)
  l2, r2, none = G.frames_u8_gpu(frames, want_rgb=False, augment=p)
  assert none is None and torch.equal(l2, want[0]) and torch.equal(r2, want[1])
  # identity factors WITH the operations enabled are the identity too, up to the contrast mean's blend with sigma = 0
  q = _params([(0, 2)] * (12 * F), [(1, 1, 1)] * (12 * F), None)
  assert torch.equal(G.frames_u8_gpu(frames, augment=q)[0], want[0])


def test_dst_slots_and_sentinel():
  H, W = 48, 32
  images, rows, frows, shifts = A.case(H, W, A.FACTOR_SETS[3])
  p = _params(rows, frows, shifts)
  dev_images = torch.from_numpy(images).to(DEV)
  straight, means = G.augment_u8_gpu(dev_images, p, return_means=True)
  slots = [9, 0, 4, 7, 1, 5, 2, 8]
  out = torch.full((11, 3, H, W), -7.0, device=DEV)
  res = HF.images_u8_augment(dev_images, p.ops, p.coef, dst=torch.tensor(slots, dtype=torch.int32, device=DEV), out=out)
  assert res is out
  for n, s in enumerate(slots):
    assert torch.equal(out[s], straight[n])
  for s in (3, 6, 10):
    assert bool((out[s] == -7.0).all())
  # a slot outside the output means "not written"
  out2 = torch.full((2, 3, H, W), -7.0, device=DEV)
  HF.images_u8_augment(dev_images, p.ops, p.coef, dst=torch.tensor([-1, 1, 2, 99, -5, 0, 7, 8], dtype=torch.int32, device=DEV), out=out2)
  assert torch.equal(out2[1], straight[1]) and torch.equal(out2[0], straight[5])
  # two slots per image: both are written, -1 (or any slot outside) is "no second copy"
  two = [[9, 3], [0, -1], [4, 10], [7, -1], [1, 99], [5, -1], [-1, 2], [-1, -1]]
  out3 = torch.full((11, 3, H, W), -7.0, device=DEV)
  HF.images_u8_augment(dev_images, p.ops, p.coef, dst=torch.tensor(two, dtype=torch.int32, device=DEV), out=out3)
  for n, row in enumerate(two):
    for s in row:
      if 0 <= s < 11:
        assert torch.equal(out3[s], straight[n]), (n, s)
  for s in (6, 8):
    assert bool((out3[s] == -7.0).all())
  with pytest.raises(ValueError):
    HF.images_u8_augment(dev_images, p.ops, p.coef, dst=torch.tensor(slots, dtype=torch.int32, device=DEV))
  with pytest.raises(ValueError):
    G.augment_u8_gpu(dev_images[:4], p)


def test_frame_layout_with_twelve_rows_per_frame():
  F, H, W = 2, 48, 32
  frames = R.frames_u8(F, H, W, 43)
  p = G.draw_colour_params(12 * F, DEV, generator=torch.Generator().manual_seed(9))
  assert len({tuple(r) for r in p.coef_host.tolist()}) == 12 * F
  left, right, rgb = G.frames_u8_gpu(torch.from_numpy(frames).to(DEV), augment=p)
  flat, means = G.augment_u8_gpu(torch.from_numpy(frames).to(DEV).view(12 * F, H, W, 3), p, return_means=True)
  _check(frames.reshape(12 * F, H, W, 3), p.ops_host.tolist(), p.coef_host[:, 0:6:2].double().tolist(), p.coef_host[:, 6:].numpy(), flat.cpu(),
         means.cpu(), A.e_ref())
  from models.mode_multiview import split_frames
  wl, wr, wrgb = split_frames(flat.view(F, 12, 3, H, W))
  assert torch.equal(left, wl) and torch.equal(right, wr) and torch.equal(rgb, wrgb)
  assert left.is_contiguous() and right.is_contiguous() and rgb.is_contiguous()


def test_repeatable_and_blind_to_the_workspace(monkeypatch):
  H, W = 96, 80
  images, rows, frows, shifts = A.case(H, W, A.FACTOR_SETS[2])
  p = _params(rows, frows, shifts)
  dev_images = torch.from_numpy(images).to(DEV)
  a, ma = G.augment_u8_gpu(dev_images, p, return_means=True)
  b, mb = G.augment_u8_gpu(dev_images, p, return_means=True)
  assert torch.equal(a, b) and torch.equal(ma, mb)
  real_empty = torch.empty

  def nan_empty(*args, **kw):  # every buffer the call allocates -- the workspace among them -- starts as NaN
    t = real_empty(*args, **kw)
    return t.fill_(float('nan')) if t.is_floating_point() else t

  monkeypatch.setattr(torch, 'empty', nan_empty)
  c, mc = G.augment_u8_gpu(dev_images, p, return_means=True)
  monkeypatch.undo()
  assert torch.equal(a, c) and torch.equal(ma, mc) and bool(torch.isfinite(c).all())


def test_graph_replay_with_new_draws():
  F, H, W = 1, 48, 32
  frames = torch.from_numpy(R.frames_u8(F, H, W, 47)).to(DEV)
  p = G.draw_colour_params(12, DEV, generator=torch.Generator().manual_seed(1))
  new = G.draw_colour_params(12, DEV, generator=torch.Generator().manual_seed(2), share=2)
  first = [t.clone() for t in G.frames_u8_gpu(frames, augment=p)]  # eager: the slot table is uploaded here
  want_new = [t.clone() for t in G.frames_u8_gpu(frames, augment=new)]
  assert not torch.equal(first[0], want_new[0])
  torch.cuda.synchronize()
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(s):
    G.frames_u8_gpu(frames, augment=p)
  torch.cuda.current_stream().wait_stream(s)
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    outs = G.frames_u8_gpu(frames, augment=p)
  g.replay()
  torch.cuda.synchronize()
  assert all(torch.equal(a, b) for a, b in zip(outs, first))
  p.copy_from(new)
  g.replay()
  torch.cuda.synchronize()
  assert all(torch.equal(a, b) for a, b in zip(outs, want_new))


def test_erp_pairs_with_augmentation():
  N, He, We, H, W = 2, 32, 64, 32, 16
  rng = np.random.RandomState(5)
  pairs = torch.from_numpy(rng.randint(0, 256, (N, 2, He, We, 3)).astype(np.uint8)).to(DEV)
  p = G.draw_colour_params(2 * N, DEV, generator=torch.Generator().manual_seed(3), share=2)
  plain = G.erp_pairs_gpu(pairs, shape=(H, W), return_u8=True)
  out = G.erp_pairs_gpu(pairs, shape=(H, W), return_u8=True, augment=p)
  assert torch.equal(out['cassini_u8'], plain['cassini_u8'])
  want = G.augment_u8_gpu(out['cassini_u8'].view(2 * N, H, W, 3), p).view(N, 2, 3, H, W)
  assert torch.equal(out['leftImg'], want[:, 0]) and torch.equal(out['rightImg'], want[:, 1])
  assert not torch.equal(out['leftImg'], plain['leftImg'])
  assert torch.equal(out['leftImg_flip'], want[:, 1].flip(3)) and torch.equal(out['rightImg_flip'], want[:, 0].flip(3))
  noflip = G.erp_pairs_gpu(pairs, shape=(H, W), flip=False, augment=p)
  assert 'leftImg_flip' not in noflip and 'cassini_u8' not in noflip and torch.equal(noflip['leftImg'], want[:, 0])
  none = G.erp_pairs_gpu(pairs, shape=(H, W), return_u8=True)  # augment=None: today's path
  assert all(torch.equal(none[k], plain[k]) for k in plain)


def test_full_size_frame():
  F, H, W = 1, 1024, 512
  frames = R.frames_u8(F, H, W, 53)
  p = G.draw_colour_params(12, DEV, generator=torch.Generator().manual_seed(4))
  dev = torch.from_numpy(frames).to(DEV)
  flat, means = G.augment_u8_gpu(dev.view(12, H, W, 3), p, return_means=True)
  left, right, rgb = G.frames_u8_gpu(dev, augment=p)
  both = torch.stack([left, right], 1).view(12, 3, H, W)
  assert torch.equal(both, flat)
  assert torch.equal(rgb.view(4, 3, H, W), flat[[0, 1, 10, 11]])
  _check(frames.reshape(12, H, W, 3), p.ops_host.tolist(), p.coef_host[:, 0:6:2].double().tolist(), p.coef_host[:, 6:].numpy(), flat.cpu(),
         means.cpu(), A.e_ref())
