"""CPU tier of the colour augmentation: the host restatement against the reference's Lighting fixture, the error the GPU
test's bound is made of, the draw helper, ColourParams' refusals and the two C-ABI entries' argument checks.  No GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import augment_ref as A
import mode_hip
from dataloader import gpu_ingest as G
from dataloader import preprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'augment_lighting.npz')


def test_lighting_is_the_references_bit_for_bit():
  """tests/golden/augment_lighting.npz is the reference's Lighting(0.1, eigval, eigvec) under a seed: the product's constants are its
  constants, lighting_shift of its alphas is its shift, and input + shift is its output."""
  z = np.load(GOLDEN)
  assert np.array_equal(G.PCA_EIGVAL.numpy(), z['eigval']) and np.array_equal(G.PCA_EIGVEC.numpy(), z['eigvec'])
  shift = G.lighting_shift(torch.from_numpy(z['alpha']))
  assert shift.dtype == torch.float32 and np.array_equal(shift.numpy(), z['shift'])
  assert np.array_equal((torch.from_numpy(z['img']) + shift.view(3, 1, 1)).numpy(), z['out'])
  # the restatement's lighting step: an image without operations, un-normalised again
  img8 = np.random.RandomState(3).randint(0, 256, (4, 8, 3)).astype(np.uint8)
  ops, coef = A.tables([()], [(1, 1, 1)], z['shift'][None])
  out, _ = A.augment(img8, ops[0], coef[0])
  x = torch.from_numpy(img8.transpose(2, 0, 1).copy()).float().div(255) + torch.from_numpy(z['shift']).view(3, 1, 1)
  want = (x - torch.tensor(A.MEAN).view(3, 1, 1)) / torch.tensor(A.STD).view(3, 1, 1)
  assert torch.equal(out, want)


def test_no_operation_and_no_shift_is_the_plain_transform():
  img8 = np.random.RandomState(4).randint(0, 256, (6, 4, 3)).astype(np.uint8)
  ops, coef = A.tables([()], [(1, 1, 1)], np.zeros((1, 3), np.float32))
  out, info = A.augment(img8, ops[0], coef[0])
  assert torch.equal(out, preprocess.get_transform_stage1(augment=False)(img8)) and info['mean'] is None


def test_e_ref_is_sane():
  """E_ref = max |float32 restatement - float64 restatement| over the GPU test's case set (tests/augment_ref.py: three sizes, four factor
  sets with the extremes 0.6 / 1.4, the six orders).  1.44e-6 was measured when the contract was written; the cap is 2^-18."""
  e = A.e_ref()
  print('E_ref = %.3e' % e)
  assert math.isfinite(e) and 0 < e < 2.0 ** -18


def test_draws_are_reproducible_and_in_range():
  a = G.draw_colour_params(24, 'cpu', generator=torch.Generator().manual_seed(5))
  b = G.draw_colour_params(24, 'cpu', generator=torch.Generator().manual_seed(5))
  c = G.draw_colour_params(24, 'cpu', generator=torch.Generator().manual_seed(6))
  assert torch.equal(a.ops_host, b.ops_host) and torch.equal(a.coef_host, b.coef_host) and not torch.equal(a.coef_host, c.coef_host)
  assert a.n == 24 and a.ops_host.dtype == torch.int32 and tuple(a.ops_host.shape) == (24, 3) and tuple(a.coef_host.shape) == (24, 9)
  assert torch.equal(a.ops, a.ops_host) and torch.equal(a.coef, a.coef_host)
  rho = a.coef_host[:, 0:6:2]
  assert float(rho.min()) >= np.float32(0.6) and float(rho.max()) <= np.float32(1.4)
  assert np.array_equal(a.coef_host[:, 1:6:2].numpy(), (1.0 - rho.numpy().astype(np.float64)).astype(np.float32))  # sigma: in double, rounded once
  assert all(sorted(r) == [0, 1, 2] for r in a.ops_host.tolist())
  assert len({tuple(r) for r in a.ops_host.tolist()}) > 1 and bool((a.coef_host[:, 6:] != 0).all())


def test_share_repeats_rows():
  g = lambda: torch.Generator().manual_seed(11)
  one = G.draw_colour_params(4, 'cpu', generator=g())
  for share, n in ((2, 7), (12, 24), (3, 3)):
    p = G.draw_colour_params(n, 'cpu', generator=g(), share=share)
    for i in range(n):
      assert torch.equal(p.ops_host[i], p.ops_host[i - i % share]) and torch.equal(p.coef_host[i], p.coef_host[i - i % share])
    assert torch.equal(p.coef_host[0], one.coef_host[0])
    if n > share:
      assert torch.equal(p.coef_host[share], one.coef_host[1]) and torch.equal(p.ops_host[share], one.ops_host[1])


def test_disabled_operations_are_skipped():
  p = G.draw_colour_params(16, 'cpu', generator=torch.Generator().manual_seed(2), contrast=None, alphastd=0)
  for r in p.ops_host.tolist():
    assert sorted(r[:2]) == [0, 2] and r[2] == G.OP_NONE  # the enabled ones first, in the drawn order; no contrast code anywhere
  assert bool((p.coef_host[:, 6:] == 0).all()) and bool((p.coef_host[:, 2] == 1).all()) and bool((p.coef_host[:, 3] == 0).all())
  q = G.draw_colour_params(3, 'cpu', brightness=None, contrast=None, saturation=None, alphastd=0)
  assert bool((q.ops_host == G.OP_NONE).all())
  assert G.draw_colour_params(0, 'cpu').n == 0


def test_draw_order_is_the_documented_one():
  """The documented calls, made here under the same seed: randperm(4); uniform_ for brightness, contrast, saturation; normal_ for the
  alphas -- per image.  (torchvision's own draw order is restated, not run: it is not installed.)"""
  torch.manual_seed(77)
  p = G.draw_colour_params(3, 'cpu')
  torch.manual_seed(77)
  for i in range(3):
    perm = torch.randperm(4).tolist()
    f = [float(torch.empty(1).uniform_(0.6, 1.4)) for _ in range(3)]
    alpha = torch.empty(3).normal_(0, 0.1)
    assert p.ops_host[i].tolist() == [c for c in perm if c != 3]
    assert np.array_equal(p.coef_host[i, 0:6:2].numpy(), np.array(f, dtype=np.float32))
    assert torch.equal(p.coef_host[i, 6:], G.lighting_shift(alpha))


def test_colour_params_refusals():
  ok = G.ColourParams([[0, 1, 2], [2]], [(1, 1, 1), (0.5, 1, 2)], None, 'cpu')
  assert ok.ops_host.tolist() == [[0, 1, 2], [2, -1, -1]] and ok.coef_host[1].tolist() == [0.5, 0.5, 1, 0, 2, -1, 0, 0, 0]
  with pytest.raises(ValueError, match='repeats'):
    G.ColourParams([[0, 0]], [(1, 1, 1)], None, 'cpu')
  with pytest.raises(ValueError, match='>= 0'):
    G.ColourParams([[0]], [(-0.1, 1, 1)], None, 'cpu')
  with pytest.raises(ValueError, match='hue'):
    G.ColourParams([[0, 3]], [(1, 1, 1)], None, 'cpu')
  with pytest.raises(ValueError, match='unknown'):
    G.ColourParams([[7]], [(1, 1, 1)], None, 'cpu')
  with pytest.raises(ValueError, match='factor rows'):
    G.ColourParams([[0], [1]], [(1, 1, 1)], None, 'cpu')
  with pytest.raises(ValueError, match='copy_from'):
    ok.copy_from(G.ColourParams([[0]], [(1, 1, 1)], None, 'cpu'))
  other = G.ColourParams([[1], [0, 2]], [(1, 0.7, 1), (1.2, 1, 0.9)], torch.ones(2, 3), 'cpu')
  ops_ptr, coef_ptr = ok.ops.data_ptr(), ok.coef.data_ptr()
  ok.copy_from(other)
  assert torch.equal(ok.ops, other.ops) and torch.equal(ok.coef, other.coef) and (ok.ops.data_ptr(), ok.coef.data_ptr()) == (ops_ptr, coef_ptr)
  # the device calls refuse a wrong n and CPU images
  with pytest.raises(ValueError, match='2 images'):
    G._require_params(ok, 3, torch.device('cpu'), 'x')
  with pytest.raises(NotImplementedError):
    G.augment_u8_gpu(torch.zeros(2, 4, 4, 3, dtype=torch.uint8), ok)
  with pytest.raises(NotImplementedError):
    G.frames_u8_gpu(torch.zeros(1, 12, 4, 4, 3, dtype=torch.uint8), augment=ok)
  with pytest.raises(NotImplementedError):  # the host transform still refuses, and says where the augmentation lives
    preprocess.get_transform_stage1(augment=True)


def test_abi_entries_are_declared_exported_and_bound():
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mode_hip.h')).read(), flags=re.S)
  lib = mode_hip.lib()
  for name in ('mode_images_u8_augment', 'mode_images_u8_augment_workspace_bytes'):
    assert re.search(r'\b%s\s*\(' % name, src) and hasattr(lib, name) and name in mode_hip.SIGNATURES
  assert 'mode_images_u8_augment_workspace_bytes' not in mode_hip.LAUNCHING and 'mode_images_u8_augment' in mode_hip.LAUNCHING
  assert mode_hip.SIGNATURES['mode_images_u8_augment'][1][-1] is ctypes.c_void_p  # the stream is the last argument
  q = lib.mode_images_u8_augment_workspace_bytes
  assert q(12, 1024, 512) == 12 * 128 * 8 and q(2, 512, 256) == 2 * 128 * 8 and q(1, 8, 12) == 8 and q(3, 48, 32) == 3 * 2 * 8 and q(0, 8, 8) == 0
  assert all(q(n, h, w) % 8 == 0 for n, h, w in ((1, 2, 2), (5, 96, 80), (7, 2048, 1024)))
  assert q(2, 2048, 1024) == q(2, 1024, 512)  # capped: a function of H W alone, a few hundred doubles per image at most


def test_argument_validation_without_gpu():
  """As tests/test_abi.py::test_argument_validation_without_gpu: refused on the host before any launch, with a message."""
  lib = mode_hip.lib()
  null, p = ctypes.c_void_p(0), ctypes.c_void_p(4096)
  f = lib.mode_images_u8_augment
  big = 1 << 20

  def refused(*args):
    rc = f(*args)
    return rc == -1 and lib.mode_last_error()

  assert b'null pointer' in refused(null, p, p, null, 1, 2, 8, 12, 2, p, null, p, big, null)
  assert b'null pointer' in refused(p, null, p, null, 1, 2, 8, 12, 2, p, null, p, big, null)
  assert b'null pointer' in refused(p, p, null, null, 1, 2, 8, 12, 2, p, null, p, big, null)
  assert b'null pointer' in refused(p, p, p, null, 1, 2, 8, 12, 2, null, null, p, big, null)
  assert b'null pointer' in refused(p, p, p, null, 1, 2, 8, 12, 2, p, null, null, big, null)
  assert b'4-byte aligned' in refused(ctypes.c_void_p(4098), p, p, null, 1, 2, 8, 12, 2, p, null, p, big, null)
  assert b'4-byte aligned' in refused(p, p, p, ctypes.c_void_p(4097), 1, 2, 8, 12, 2, p, null, p, big, null)
  assert b'16-byte aligned' in refused(p, p, p, null, 1, 2, 8, 12, 2, ctypes.c_void_p(4104), null, p, big, null)
  assert b'8-byte aligned' in refused(p, p, p, null, 1, 2, 8, 12, 2, p, null, ctypes.c_void_p(4100), big, null)
  assert b'slots per image' in refused(p, p, p, p, 3, 2, 8, 12, 2, p, null, p, big, null)
  assert b'multiple of 4' in refused(p, p, p, null, 1, 2, 3, 5, 2, p, null, p, big, null)
  assert b'bad size' in refused(p, p, p, null, 1, 2, 0, 12, 2, p, null, p, big, null)
  assert b'bad size' in refused(p, p, p, null, 1, -1, 8, 12, 2, p, null, p, big, null)
  assert b'too large' in refused(p, p, p, null, 1, 1366, 1024, 512, 2, p, null, p, 1 << 30, null)   # 3 N H W >= 2^31
  assert b'too large' in refused(p, p, p, null, 1, 2, 1024, 512, 1366, p, null, p, 1 << 30, null)   # 3 slots H W >= 2^31
  assert b'too large' in refused(p, p, p, null, 1, 1, 65536, 65536, 1, p, null, p, 1 << 30, null)
  need = lib.mode_images_u8_augment_workspace_bytes(2, 48, 32)
  assert b'workspace' in refused(p, p, p, null, 1, 2, 48, 32, 2, p, null, p, need - 8, null)
  assert f(null, null, null, null, 1, 0, 8, 12, 0, null, null, null, 0, null) == 0  # N = 0: a no-op


def test_the_library_has_no_memset():
  src = open(os.path.join(ROOT, 'mode-2022_amd', 'csrc', 'augment.hip')).read()
  assert 'hipMemset' not in src and 'atomic' not in re.sub(r'//.*', '', src)
