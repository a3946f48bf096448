"""BatchNorm backward behind a residual add + ReLU: the masked gradient is written ONCE (csrc/bn_act.hip, mode_bn_train_bwd_amax).

With `gadd` and the mask taken from the forward output (mode 1), bn_bwd_stats_kernel stores g = out > 0 ? gout : 0 to gadd while it
sums, and the apply pass reads (gadd, y) instead of (gout, y, out) and writes gy only: 7 tensor passes instead of 8.  The path without
gadd is the code it always was, so gy / ggamma / gbeta of the two calls must agree in every bit; gadd is the masked gradient exactly;
gy is held against a float64 torch BatchNorm + add + ReLU backward under the bound of tests/test_gpu_kernels.py::
test_bn_act_train_and_eval (5e-5 relative to the largest reference gradient; no element of these seeded inputs is within 1e-5 of the
ReLU threshold, asserted, so none may legitimately fall on the other side in fp32).

Shapes (B, C, S): (2, 3, 7) the scalar path (rows not 16-byte multiples); (4, 5, 16384) the 4x-unrolled 16-byte loop with two
statistics blocks per row; (4, 6, 1028) with two statistics groups (one block per row, the tail loop of the 16-byte path); (1, 2, 1031)
the scalar path with four or five elements per thread (its unrolled body and its remainder)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mode_hip
from mode_hip import functional as HF

DEV = 'cuda:0'
CASES = [((2, 3, 7), 1), ((4, 5, 16384), 1), ((4, 6, 1028), 2), ((1, 2, 1031), 1)]
EPS = 1e-5
SEED = 74  # (of the generators below: chosen so that no pre-ReLU value of any case lies within 1e-5 of zero, see _case)


def _rand(shape, seed, scale=1.0):
  return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _case(shape, groups, seed=SEED):
  """Seeded inputs and the float64 reference (computed once per case, shared by both parametrisations, never modified)."""
  B, C, S = shape
  y = _rand(shape, seed, 2.0) + 1.5
  add = _rand(shape, seed + 1)
  gout = _rand(shape, seed + 2)
  g = torch.Generator().manual_seed(7)
  gamma = 1 + 0.2 * torch.randn(C, generator=g)
  beta = 0.3 * torch.randn(C, generator=g)
  ya = y.double().requires_grad_(True)
  outs = []
  for part, apart in zip(ya.chunk(groups, 0), add.double().chunk(groups, 0)):  # a statistics group = one call of the module
    outs.append(torch.nn.functional.batch_norm(part, None, None, gamma.double(), beta.double(), True, 0.1, EPS) + apart)
  pre = torch.cat(outs, 0)
  torch.relu(pre).backward(gout.double())
  assert int((pre.detach().abs() < 1e-5).sum()) == 0, 'an input element sits on the ReLU threshold: choose other seeds'
  return {'y': y, 'add': add, 'gout': gout, 'gamma': gamma, 'beta': beta, 'gy_ref': ya.grad.detach()}


def _ptr(t):
  return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _backward(c, shape, groups, with_gadd, with_amax):
  """Forward through mode_bn_train_fwd (add + ReLU), then ONE call of mode_bn_train_bwd_amax in mode 1; returns device tensors."""
  lib = mode_hip.lib()
  B, C, S = shape
  y, add, gout, gamma, beta = (c[k].to(DEV) for k in ('y', 'add', 'gout', 'gamma', 'beta'))
  out = torch.empty_like(y)
  mean = torch.empty(groups * C, device=DEV)
  invstd = torch.empty_like(mean)
  ws = torch.empty(lib.mode_bn_workspace_bytes(C * groups) // 4, device=DEV)
  rc = lib.mode_bn_train_fwd(_ptr(y), _ptr(add), _ptr(gamma), _ptr(beta), None, None, None, 0.1, EPS, 1, _ptr(out), _ptr(mean), _ptr(invstd),
                             None, None, _ptr(ws), B, C, S, groups, None)
  assert rc == 0, lib.mode_last_error()
  gy = torch.full_like(y, float('nan'))
  gadd = torch.full_like(y, float('nan')) if with_gadd else None
  ggamma, gbeta = torch.full_like(gamma, float('nan')), torch.full_like(gamma, float('nan'))
  amax = torch.full((HF.BN_ABSMAX_FLOATS,), float('nan'), device=DEV) if with_amax else None
  rc = lib.mode_bn_train_bwd_amax(_ptr(gout), _ptr(y), _ptr(out), _ptr(gamma), _ptr(mean), _ptr(invstd), None, None, 1, _ptr(gy), _ptr(gadd),
                                  _ptr(ggamma), _ptr(gbeta), 0, _ptr(ws), B, C, S, groups, _ptr(amax), None)
  assert rc == 0, lib.mode_last_error()
  torch.cuda.synchronize()
  return {'gy': gy, 'gadd': gadd, 'ggamma': ggamma, 'gbeta': gbeta, 'amax': amax, 'out': out, 'gout': gout}


@pytest.mark.gpu
@pytest.mark.parametrize('with_amax', [False, True])
@pytest.mark.parametrize('shape,groups', CASES)
def test_bn_backward_writes_the_skip_gradient_once(shape, groups, with_amax):
  c = _case(shape, groups)
  plain = _backward(c, shape, groups, False, with_amax)
  fused = _backward(c, shape, groups, True, with_amax)
  for k in ('gy', 'ggamma', 'gbeta'):
    assert torch.equal(fused[k], plain[k]), '%s differs between the call with gadd and the call without' % k
  assert torch.equal(fused['gadd'], torch.where(fused['out'] > 0, fused['gout'], torch.zeros_like(fused['gout'])))
  if with_amax:  # the maximum of gy comes out of the apply pass on both routes
    assert torch.equal(fused['amax'], plain['amax'])
    assert float(fused['amax'].max()) == float(fused['gy'].abs().max())
  ref = c['gy_ref']
  err = float((fused['gy'].cpu().double() - ref).abs().max())
  bound = 5e-5 * max(1.0, float(ref.abs().max()))
  print('bn_train_bwd %s groups %d: max |gy - float64| = %.3e, bound %.3e' % (shape, groups, err, bound))
  assert err < bound


def test_bn_backward_refuses_an_aliased_skip_gradient():
  """gadd is written by the statistics pass and read back by the apply pass: gadd == gout / y / out (or a range that overlaps one of
  them) is rejected on the host, before any launch (made-up addresses: nothing is dereferenced)."""
  lib = mode_hip.lib()
  B, C, S = 2, 4, 64  # 2 KB per tensor
  gout, y, out, gy, free, small = (ctypes.c_void_p(a) for a in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000))

  def call(gadd):
    return lib.mode_bn_train_bwd_amax(gout, y, out, small, small, small, None, None, 1, gy, gadd, small, small, 0, free, B, C, S, 1, None, None)

  for gadd in (gout, y, out, ctypes.c_void_p(0x20000 + 16), ctypes.c_void_p(0x30000 - 16)):
    assert call(gadd) == -1 and b'gadd aliases' in lib.mode_last_error(), hex(gadd.value)
