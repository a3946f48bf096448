"""8-bit ingest, CPU tier: the host-built tables against Pillow and the host transform, a numpy stand-in of the ingest kernel
against split_frames, the refusals of ModeMultiView(resize=True), and the host-side argument checks of the three C-ABI entries (no
launch)."""
import ctypes
import subprocess
import sys

import numpy as np
import pytest
import torch

import ingest_ref as R
import mode_hip
import models
from dataloader import gpu_ingest, preprocess
from mode_hip import functional as HF
from models import mode_multiview


@pytest.mark.parametrize('size', [(32, 16), (64, 48), (1024, 512)])  # (h, w)
def test_table_builder_reproduces_pillow_bit_for_bit(size):
  h, w = size
  for kind, a in R.images(h, w, 7 + h).items():
    want = R.pil_half(a)
    clipped = [0, 0]
    got = R.pil_half_numpy(a, clipped)
    assert want.shape == got.shape == (h // 2, w // 2, 3)
    assert int((got != want).sum()) == 0, (kind, int((got != want).sum()))
    if kind == 'binary':
      assert clipped[0] > 0 and clipped[1] > 0 and want.min() == 0 and want.max() == 255  # the clip is taken at both ends


def test_table_structure():
  """8 taps at stride 2 in the interior, two shorter rows at each edge: five distinct coefficient rows; sum |kk| keeps 32 bits enough."""
  for n in (16, 32, 512, 1024):
    xmin, count, kk = preprocess.pil_half_table(n)
    i = np.arange(n // 2)
    assert np.array_equal(xmin, np.maximum(0, 2 * i - 3)) and np.array_equal(xmin + count, np.minimum(n, 2 * i + 5))
    assert count.max() == 8 and len({tuple(r) for r in kk.tolist()}) == 5
    assert all(not kk[r, count[r]:].any() for r in range(n // 2))
    assert 255 * int(np.abs(kk.astype(np.int64)).sum(1).max()) + (1 << 21) < 2 ** 31
    assert (np.abs(kk.sum(1) - (1 << 22)) <= 4).all()  # rows are normalised before the rounding
    # what the kernel's tile assumes: 16 output rows reach 38 input rows, 32 output columns 70 input columns
    for t, span in ((16, 38), (32, 70)):
      for i0 in range(0, n // 2, t):
        last = min(i0 + t, n // 2) - 1
        assert xmin[last] + count[last] - xmin[i0] <= span and (xmin[i0:last + 1] >= xmin[i0]).all()
    rows = gpu_ingest.half_table_rows(n)
    assert rows.dtype == torch.int32 and tuple(rows.shape) == (n // 2, 10) and rows.is_contiguous()
    assert np.array_equal(rows[:, 0].numpy(), xmin) and np.array_equal(rows[:, 1].numpy(), count) and np.array_equal(rows[:, 2:].numpy(), kk)
  for bad in (0, 1, 33, -4):
    with pytest.raises(ValueError):
      preprocess.pil_half_table(bad)


def test_normalisation_table_is_the_host_transform():
  lut = preprocess.norm_table()
  assert lut.dtype == torch.float32 and tuple(lut.shape) == (256, 3) and lut.is_contiguous()
  ramp = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)  # (1, 256, 3): all 256 values in each channel
  want = preprocess.get_transform_stage1(augment=False)(ramp)  # (3, 1, 256)
  assert torch.equal(lut, want[:, 0, :].t())
  # and a lookup has the bits of the transform on an arbitrary image
  a = R.images(6, 10, 3)['random']
  assert torch.equal(torch.from_numpy(np.stack([lut.numpy()[a[..., c], c] for c in range(3)])), R.host_norm(a))


def test_numpy_stand_in_of_the_ingest_is_split_frames():
  frames = R.frames_u8(2, 6, 10, 11)
  left, right, rgb = R.ingest_numpy(frames, preprocess.norm_table())
  wl, wr, wrgb = R.host_split(frames)
  assert torch.equal(left, wl) and torch.equal(right, wr) and torch.equal(rgb, wrgb)


def _tiny(**kw):
  return models.ModeMultiView(16, 10., 64, 32, channels=(8, 16, 32, 64), **kw)


def test_resize_refusals_and_defaults():
  assert _tiny().resize is False and _tiny(resize=True).resize is True
  import inspect
  assert inspect.signature(models.ModeMultiView.__init__).parameters['resize'].default is False
  net = _tiny(resize=True).eval()
  with pytest.raises(ValueError, match='8-bit images'):  # float frames: refused with the reason, on any device
    net(torch.zeros(1, 12, 3, 64, 32))
  # uint8 CPU frames raise as float CPU frames do
  for n in (net, _tiny().eval()):
    with pytest.raises(NotImplementedError):
      n(torch.zeros(1, 12, 64, 32, 3, dtype=torch.uint8))
  with pytest.raises(NotImplementedError):
    _tiny().eval()(torch.zeros(1, 12, 3, 64, 32))
  with pytest.raises(RuntimeError, match='inference only'):
    _tiny(resize=True).train()(torch.zeros(1, 12, 64, 32, 3, dtype=torch.uint8))


def test_resize_sizes_follow_the_pooling_depth():
  assert mode_multiview.fusion_size_multiple(_tiny().fusion) == 8  # three poolings on the depth branch
  assert mode_multiview.fusion_size_multiple(_tiny(fusion='Baseline').fusion) == 1
  for h, w in ((72, 40), (64, 40), (72, 32)):  # half of it is no multiple of 8
    with pytest.raises(ValueError, match='multiple of 16'):
      models.ModeMultiView(16, 10., h, w, resize=True)
  assert models.ModeMultiView(16, 10., 64, 32, resize=True, fusion='Baseline').resize


def test_public_functions_refuse_what_is_not_contiguous_uint8_on_the_gpu():
  for fn in (gpu_ingest.frames_u8_gpu, gpu_ingest.rgb_half_gpu):
    with pytest.raises(TypeError, match='uint8'):
      fn(torch.zeros(1, 12, 4, 4, 3))
    with pytest.raises(TypeError):
      fn(np.zeros((1, 12, 4, 4, 3), dtype=np.uint8))
    with pytest.raises(NotImplementedError):
      fn(torch.zeros(1, 12, 4, 4, 3, dtype=torch.uint8))
  for fn in (lambda: HF.decimate2(torch.zeros(2, 4, 4)), lambda: HF.frames_u8_ingest(torch.zeros(1, 12, 4, 4, 3, dtype=torch.uint8), torch.zeros(256, 3)),
             lambda: HF.rgb_half_pil(torch.zeros(1, 12, 4, 4, 3, dtype=torch.uint8), torch.zeros(2, 10), torch.zeros(2, 10), torch.zeros(256, 3))):
    with pytest.raises(NotImplementedError):
      fn()


def test_importing_the_module_loads_no_native_library():
  code = ('import sys\nsys.path[:0] = %r\nimport mode_hip\nfrom dataloader import gpu_ingest, preprocess\n'
          'assert mode_hip._lib is None\npreprocess.pil_half_table(32); preprocess.norm_table(); gpu_ingest.half_table_rows(16)\n'
          'assert mode_hip._lib is None\n' % ([p for p in sys.path if p],))
  subprocess.run([sys.executable, '-c', code], check=True)


def test_ingest_entries_validate_on_the_host():
  """NULL pointers, bad sizes, misalignment and element counts >= 2^31 are refused before any launch; F = 0 is a no-op."""
  lib = mode_hip.lib()
  null, one, odd = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(4098)

  def ingest(frames=one, lut=one, F=1, H=16, W=8, left=one, right=one, rgb=one):
    return lib.mode_frames_u8_ingest(frames, lut, F, H, W, left, right, rgb, null)

  assert ingest(F=-1) == -1 and b'bad size' in lib.mode_last_error()
  assert ingest(H=0) == -1 and ingest(W=-2) == -1
  assert ingest(H=3, W=6) == -1 and b'multiple of 4' in lib.mode_last_error()
  assert ingest(F=60, H=1024, W=1024) == -1 and b'too large' in lib.mode_last_error()  # 36 F H W >= 2^31
  assert ingest(F=1 << 30, H=1 << 20, W=1 << 20) == -1 and b'too large' in lib.mode_last_error()
  for kw in ('frames', 'lut', 'left', 'right'):
    assert ingest(**{kw: null}) == -1 and b'null pointer' in lib.mode_last_error(), kw
  assert ingest(frames=odd) == -1 and b'aligned' in lib.mode_last_error()
  for kw in ('left', 'right', 'rgb'):
    assert ingest(**{kw: ctypes.c_void_p(4104)}) == -1 and b'aligned' in lib.mode_last_error(), kw
  assert ingest(F=0, frames=null, lut=null, left=null, right=null, rgb=null) == 0

  def half(frames=one, tw=one, th=one, lut=one, F=1, H=16, W=8, out=one, u8=one):
    return lib.mode_rgb_half_pil(frames, tw, th, lut, F, H, W, out, u8, null)

  assert half(F=-1) == -1 and half(H=0) == -1 and half(W=0) == -1 and b'bad size' in lib.mode_last_error()
  assert half(H=15) == -1 and b'even' in lib.mode_last_error()
  assert half(W=7) == -1 and b'even' in lib.mode_last_error()
  assert half(F=60, H=1024, W=1024) == -1 and b'too large' in lib.mode_last_error()
  for kw in ('frames', 'tw', 'th', 'lut', 'out'):
    assert half(**{kw: null}) == -1 and b'null pointer' in lib.mode_last_error(), kw
  for kw in ('frames', 'tw', 'th'):
    assert half(**{kw: odd}) == -1 and b'aligned' in lib.mode_last_error(), kw
  assert half(F=0, frames=null, tw=null, th=null, lut=null, out=null, u8=null) == 0

  two = ctypes.c_void_p(8192)
  assert lib.mode_decimate2(one, two, -1, 4, 4, null) == -1 and b'bad size' in lib.mode_last_error()
  assert lib.mode_decimate2(one, two, 1, 0, 4, null) == -1 and lib.mode_decimate2(one, two, 1, 4, -1, null) == -1
  assert lib.mode_decimate2(one, two, 1 << 11, 1024, 1024, null) == -1 and b'too large' in lib.mode_last_error()
  assert lib.mode_decimate2(one, two, 1 << 40, 1 << 20, 1 << 20, null) == -1 and b'too large' in lib.mode_last_error()
  assert lib.mode_decimate2(null, two, 1, 4, 4, null) == -1 and b'null pointer' in lib.mode_last_error()
  assert lib.mode_decimate2(one, null, 1, 4, 4, null) == -1 and b'null pointer' in lib.mode_last_error()
  assert lib.mode_decimate2(one, one, 1, 4, 4, null) == -1 and b'in-place' in lib.mode_last_error()
  assert lib.mode_decimate2(null, null, 0, 4, 4, null) == 0
