"""The spatial pyramid pooling operators of the conv='Regular' extractor (csrc/spp.hip; HF.spp_pool, HF.spp_concat): values and
gradients against float64, bit repeatability, and the host-side refusals of the four C-ABI entries.

Yardstick: the reference's composition -- F.avg_pool2d(k, k), F.interpolate(mode='bilinear', align_corners=True), torch.cat -- in float64
on the CPU, gradients by autograd.  Tolerance, per output and per gradient: the kernel's maximum error against float64 may be at most
2 x the maximum error of torch's OWN fp32 GPU operators on the same inputs against the same float64 (only the summation order
legitimately differs: hence 2), with a floor of one fp32 ulp of the tensor's largest magnitude.  Both errors are printed.

Shapes: N = 2, (Cr, Cs, Cb) = (3, 8, 4) -- channel offsets that are multiples of nothing convenient -- and
  (64, 64)    1 x 1 at k = 64: the degenerate scale 0 (a 1-pixel source axis broadcasts); both adjoint kernels (wave, workgroup)
  (72, 136)   floor cropping in both axes: 9 x 17 blocks at k = 8 against 4 x 8 at k = 16; a ragged last 64 x 64 region
  (128, 64)   two source rows against one source column at k = 64
  (64, 66)    a width that is no multiple of 4: the kernels' one-float-per-lane form (rows cannot move 16 bytes per lane), and two
              columns that belong to no block of any level.
Three compositions per shape: the pooling alone, the concatenation alone, and the block without its convolutions (the pooled tensors'
first Cb channels go straight into the concatenation), where `skip` has both consumers and its gradient is written in one pass."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mode_hip
from mode_hip import functional as HF
from test_gpu_repeat import PoisoningLib

DEV = 'cuda:0'
N, CR, CS, CB = 2, 3, 8, 4
SHAPES = [(64, 64), (72, 136), (128, 64), (64, 66)]
KS = (8, 16, 32, 64)
WHAT = ['pool', 'concat', 'block']


def _inputs(H, W):
  g = torch.Generator().manual_seed(1000 * H + W)
  t = {'raw': torch.randn(N, CR, H, W, generator=g), 'skip': torch.randn(N, CS, H, W, generator=g)}
  for k in KS:
    t['b%d' % k] = torch.randn(N, CB, H // k, W // k, generator=g)
    t['gp%d' % k] = torch.randn(N, CS, H // k, W // k, generator=g)  # upstream gradients of the pooled tensors
  t['gcat'] = torch.randn(N, CR + CS + 4 * CB, H, W, generator=g)
  return t


def _ref_pool(x):
  return [F.avg_pool2d(x, (k, k), stride=(k, k)) for k in KS]


def _ref_concat(raw, skip, bs):
  return torch.cat([raw, skip] + [F.interpolate(b, skip.shape[2:], mode='bilinear', align_corners=True) for b in bs], 1)


def _own_pool(x):
  return list(HF.spp_pool(x))


def _own_concat(raw, skip, bs):
  return HF.spp_concat(raw, skip, *bs)


def _compose(what, t, pool, concat, own):
  """{name: tensor} of outputs and gradients of one composition on the tensors t (leaves are made here)."""
  leaf = {k: v.clone().requires_grad_(True) for k, v in t.items() if not k.startswith('g')}
  out = {}
  if what == 'pool':
    ps = pool(leaf['skip'])
    loss = sum((p * t['gp%d' % k]).sum() for p, k in zip(ps, KS))
    for p, k in zip(ps, KS):
      out['pool%d' % k] = p
    wrt = ['skip']
  elif what == 'concat':
    cat = concat(leaf['raw'], leaf['skip'], [leaf['b%d' % k] for k in KS])
    loss = (cat * t['gcat']).sum()
    out['cat'] = cat
    wrt = ['raw', 'skip'] + ['b%d' % k for k in KS]
  else:
    if own:
      ps = HF.spp_pool(leaf['skip'])
      skip = ps.skip
    else:
      ps, skip = pool(leaf['skip']), leaf['skip']
    cat = concat(leaf['raw'], skip, [p[:, :CB].contiguous() for p in ps])
    loss = (cat * t['gcat']).sum()
    out['cat'] = cat
    wrt = ['raw', 'skip']
  grads = torch.autograd.grad(loss, [leaf[k] for k in wrt])
  out.update({'g_' + k: g for k, g in zip(wrt, grads)})
  return {k: v.detach() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _truth(H, W, what):
  """float64 on the CPU, computed once per (shape, composition) and shared."""
  t = {k: v.double() for k, v in _inputs(H, W).items()}
  return _compose(what, t, _ref_pool, _ref_concat, False)


def _on_gpu(H, W, what, own):
  t = {k: v.to(DEV) for k, v in _inputs(H, W).items()}
  out = _compose(what, t, _own_pool if own else _ref_pool, _own_concat if own else _ref_concat, own)
  torch.cuda.synchronize()
  return out


def _bits_equal(a, b):
  assert a.keys() == b.keys()
  for k in a:
    assert torch.equal(a[k].contiguous().view(torch.int32), b[k].contiguous().view(torch.int32)), k


@pytest.mark.gpu
@pytest.mark.parametrize('what', WHAT)
@pytest.mark.parametrize('H,W', SHAPES)
def test_values_and_gradients_against_float64(H, W, what):
  truth = _truth(H, W, what)
  own, vendor = _on_gpu(H, W, what, True), _on_gpu(H, W, what, False)
  assert own.keys() == truth.keys()
  bad = []
  for k, want in truth.items():
    assert tuple(own[k].shape) == tuple(want.shape), k
    e_own = float((own[k].cpu().double() - want).abs().max())
    e_torch = float((vendor[k].cpu().double() - want).abs().max())
    ulp = float(np.spacing(np.float32(want.abs().max())))
    bound = max(2 * e_torch, ulp)
    print('  %s %dx%d %-8s own %.3e  torch fp32 %.3e  ulp(max) %.3e  bound %.3e' % (what, H, W, k, e_own, e_torch, ulp, bound))
    if not e_own <= bound:
      bad.append((k, e_own, bound))
  assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize('what', WHAT)
@pytest.mark.parametrize('H,W', SHAPES)
def test_two_calls_and_poisoned_calls_give_the_same_bits(H, W, what, monkeypatch):
  """Outputs and gradients: a second call, and calls behind mode_debug_poison with two different patterns (every kernel starts from
  LDS and registers full of the pattern, as tests/test_gpu_repeat.py does for the whole step), reproduce the first call bit for bit."""
  first = _on_gpu(H, W, what, True)
  _bits_equal(first, _on_gpu(H, W, what, True))
  real = mode_hip.lib()
  for pattern in (0x7fc00000, 0x3f803f80):
    proxy = PoisoningLib(real, pattern)
    monkeypatch.setattr(mode_hip, '_lib', proxy)
    try:
      again = _on_gpu(H, W, what, True)
    finally:
      monkeypatch.setattr(mode_hip, '_lib', real)
    assert proxy.calls >= 2
    _bits_equal(first, again)


@pytest.mark.gpu
def test_wrappers_refuse_what_the_kernels_do_not_take():
  x = torch.randn(1, 2, 63, 64, device=DEV)
  with pytest.raises(RuntimeError, match='at least 64 x 64'):
    HF.spp_pool(x)
  with pytest.raises(TypeError):
    HF.spp_pool(torch.randn(1, 2, 64, 64, device=DEV).double())
  with pytest.raises(ValueError):
    HF.spp_pool(torch.randn(1, 2, 64, 128, device=DEV)[:, :, :, ::2])
  with pytest.raises(NotImplementedError):
    HF.spp_pool(torch.randn(1, 2, 64, 64))
  t = {k: v.to(DEV) for k, v in _inputs(64, 64).items()}
  with pytest.raises(ValueError, match='k = 16 branch'):
    HF.spp_concat(t['raw'], t['skip'], t['b8'], t['b8'], t['b32'], t['b64'])


def test_argument_validation_without_gpu():
  """CPU tier (like test_abi.test_argument_validation_without_gpu): bad arguments are refused on the host, with a message, before
  any launch -- H = 63, null pointers, non-positive extents, a channel range outside the concatenation's gradient."""
  lib = mode_hip.lib()
  null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
  err = lib.mode_last_error
  # H (or W) below 64: the k = 64 level would have no block
  assert lib.mode_spp_pool_fwd(one, one, one, one, one, 4, 63, 64, null) == -2 and b'at least 64 x 64' in err()
  assert lib.mode_spp_pool_fwd(one, one, one, one, one, 4, 64, 63, null) == -2 and b'at least 64 x 64' in err()
  assert lib.mode_spp_pool_bwd(one, 8, 0, one, one, one, one, one, 2, 8, 63, 64, null) == -2 and b'at least 64 x 64' in err()
  assert lib.mode_spp_concat_fwd(one, one, one, one, one, one, one, 2, 3, 8, 4, 63, 64, null) == -2 and b'at least 64 x 64' in err()
  assert lib.mode_spp_concat_bwd(one, one, one, one, one, one, 2, 3, 8, 4, 64, 63, null) == -2 and b'at least 64 x 64' in err()
  # non-positive extents
  assert lib.mode_spp_pool_fwd(one, one, one, one, one, 4, 0, 64, null) == -1 and b'non-positive' in err()
  assert lib.mode_spp_pool_fwd(one, one, one, one, one, -1, 64, 64, null) == -1 and b'negative' in err()
  assert lib.mode_spp_pool_bwd(one, 8, 0, one, one, one, one, one, 2, 0, 64, 64, null) == -1 and b'bad sizes' in err()
  assert lib.mode_spp_concat_fwd(one, one, one, one, one, one, one, 2, 3, 8, 0, 64, 64, null) == -1 and b'bad sizes' in err()
  assert lib.mode_spp_concat_fwd(one, one, one, one, one, one, one, 2, 3, 8, 4, 64, -64, null) == -1 and b'non-positive' in err()
  assert lib.mode_spp_concat_bwd(one, one, one, one, one, one, -2, 3, 8, 4, 64, 64, null) == -1 and b'bad sizes' in err()
  # null pointers
  assert lib.mode_spp_pool_fwd(null, one, one, one, one, 4, 64, 64, null) == -1 and b'null pointer' in err()
  assert lib.mode_spp_pool_fwd(one, one, one, one, null, 4, 64, 64, null) == -1 and b'null pointer' in err()
  assert lib.mode_spp_pool_bwd(one, 8, 0, one, null, one, one, one, 2, 8, 64, 64, null) == -1 and b'null pointer' in err()
  assert lib.mode_spp_pool_bwd(one, 8, 0, one, one, one, one, null, 2, 8, 64, 64, null) == -1 and b'null pointer' in err()
  assert lib.mode_spp_concat_fwd(one, null, one, one, one, one, one, 2, 3, 8, 4, 64, 64, null) == -1 and b'null pointer' in err()
  assert lib.mode_spp_concat_fwd(one, one, one, one, one, one, null, 2, 3, 8, 4, 64, 64, null) == -1 and b'null pointer' in err()
  assert lib.mode_spp_concat_bwd(null, one, one, one, one, one, 2, 3, 8, 4, 64, 64, null) == -1 and b'null pointer' in err()
  assert lib.mode_spp_concat_bwd(one, one, one, null, one, one, 2, 3, 8, 4, 64, 64, null) == -1 and b'null pointer' in err()
  # the slice of mode_spp_pool_bwd must lie inside gcat's channels
  assert lib.mode_spp_pool_bwd(one, 10, 3, one, one, one, one, one, 2, 8, 64, 64, null) == -1 and b'outside' in err()
  # size limits: the plane index is a grid dimension
  assert lib.mode_spp_concat_fwd(one, one, one, one, one, one, one, 300, 64, 128, 32, 64, 64, null) == -2 and b'65535' in err()
  assert lib.mode_spp_pool_fwd(one, one, one, one, one, 4, 1 << 15, 1 << 15, null) == -2 and b'2^30' in err()
  # nothing to do: no launch, no pointer looked at
  assert lib.mode_spp_pool_fwd(null, null, null, null, null, 0, 64, 64, null) == 0
  assert lib.mode_spp_concat_bwd(null, null, null, null, null, null, 0, 3, 8, 4, 64, 64, null) == 0
