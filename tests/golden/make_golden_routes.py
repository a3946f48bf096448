#!/usr/bin/env python3
"""Which C entries mode_hip.functional calls, with which arguments, taken on the GPU at the commit BEFORE the kernel choice of every
layer family was written once (_conv3d_route, _conv2d_route, _sphere_fwd_route in functional.py).

  python tests/golden/make_golden_routes.py     # writes routes_parent.json (needs the MI355X)

That change is Python only: it moves no kernel and no launch, so the output bits are pinned already (tests/test_gpu_conv3d_bits.py,
tests/test_gpu_sphere_win_bits.py).  What those cannot see is a layer that quietly runs on another entry, a maximum pass that appears
or disappears, or a profiling label / byte count that bench.py keys on and that changed.  So this file records, per case, through
spies on functional.lib, functional.abs_max and profiling.region (profiling enabled):
  ['region', label, bytes, flops]     every profiling region, in order
  ['call', entry, [arguments]]        every launching entry (and mode_weight_pack_reuse): scalars as they are, a pointer as 'P' or '0'
                                      (null), a folded-BatchNorm epilogue as ['E', relu, has a residual]; the stream is left out
  ['amax', shape]                     every maximum pass functional.abs_max runs
Entries that launch nothing (workspace sizes, predicates, the cached table builders) are not recorded: how often a predicate is asked
is exactly what the rewrite changes.  tests/test_gpu_routes.py replays the cases and requires equality: operator cases as sequences,
the two model cases as counts per event.  Do not regenerate this file together with a change of the dispatch -- it pins the parent's.

Switch sets: 'default'; 'bf16' = CONV_ARITH 'bf16x6' with every *_F16 switch off; 'f32' = CONV_ARITH 'f32'.
Operator cases (shapes (B, Ci, Co, ...) as in make_golden_conv3d_bits.py): see OPS below; every eval case runs twice on the same
BatchNorm module, so that the second run shows the packed-weight cache hit (mode_weight_pack_reuse) under that layer's tag.
Sphere cases: SphereConv 32 -> 32 on the (128, 256) Cassini table and on the ERP table, a training step and an eval forward, under
the settings of SPHERE below; each also records what supports_transposed_io (sphere_t_supported) answers.
Model cases: one training step and one eval forward of ModeDisparity(16, 'Sphere', 64, 32, 'Cassini') at B = 1.

A second, separate case list (GRAD_CASES) pins the routes of the two spherical GRADIENTS, which the list above runs under none of their
own switches: taken at the commit BEFORE those routes were written once (_sphere_bwd_data_route, _sphere_bwd_data_t_route,
_sphere_bwd_weight_route), with this recorder run against that commit's functional.py.

  python tests/golden/make_golden_routes.py sphere_grad     # writes routes_parent_sphere_grad.json (needs the MI355X)

Its cases: the training step of the same SphereConv on both table types, both floors at 0, under SPHERE_BWD_DATA = 'scatter', under
SPHERE_BWD_DATA_T = False and under SPHERE_BWD_WEIGHT = 'gather'; and one stride-2 layer (kernel 3, stride 2, pad 1) of each type."""
import collections
import ctypes
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, 'mode-2022_amd'), HERE):
  if p not in sys.path:
    sys.path.insert(0, p)

OUT = os.path.join(HERE, 'routes_parent.json')
OUT_GRAD = os.path.join(HERE, 'routes_parent_sphere_grad.json')
DEV = 'cuda:0'

F16_SWITCHES = ('CONV3D_S1_F16', 'CONV3D_EVAL_F16', 'CONV2D_EVAL_F16', 'CONV2D_F16', 'SPHERE_FWD_F16', 'SPHERE_BWD_F16')
SWITCH_SETS = {
    'default': {'CONV_ARITH': 'bf16x6'},
    'bf16': dict({'CONV_ARITH': 'bf16x6'}, **{k: False for k in F16_SWITCHES}),
    'f32': {'CONV_ARITH': 'f32'},
}

S1 = (1, 32, 32, 6, 10, 40)
S2 = (1, 32, 64, 4, 8, 64)
DECONV = (1, 64, 32, 6, 16, 32)
ODD = (2, 20, 40, 5, 7, 33)
CO1 = (1, 20, 1, 3, 5, 33)
C2D = (2, 32, 32, 16, 32)
C2D_OFF = (1, 24, 40, 9, 33)

OPS = ([('c3d_' + op, 1, S1) for op in ('fwd', 'bwd_data', 'bwd_data_acc', 'bwd_weight', 'bwd_weight_into', 'fn_tagged', 'fn_untagged', 'eval')] +
       [('c3d_' + op, 2, S2) for op in ('fwd', 'bwd_data', 'bwd_weight', 'eval')] +
       [('deconv_fn', 2, DECONV), ('deconv_eval', 2, DECONV)] +
       [('c3d_' + op, 1, s) for s in (ODD, CO1) for op in ('fwd', 'bwd_data', 'bwd_weight')] + [('c3d_eval', 1, ODD)] +
       [('cost_conv_eval', 1, (1, 32, 32, 4, 16, 8))] +
       [('c2d_' + op, d, s) for s, dils in ((C2D, (1, 2)), (C2D_OFF, (1,))) for d in dils for op in ('fwd', 'bwd_data_acc', 'bwd_weight_into', 'eval')] +
       [('bn_act', 1, s) for s in ((1, 32, 3, 5, 8), (2, 16, 8, 12), (2, 24, 8, 12))] +
       [('classif', 1, (1, 32, 4, 6, 16))])

# (name, module switches of the setting); the windowed kernels are reached at B = 1 only with the two workgroup floors at 0
WG0 = {'SPHERE_FWD_MIN_WG': 0, 'SPHERE_BWD_SPLIT_MIN_WG': 0}
SPHERE = [('wg0', WG0), ('wg200', {'SPHERE_FWD_MIN_WG': 200}), ('gather', dict(WG0, SPHERE_FWD='gather')),
          ('nchw', dict(WG0, SPHERE_LAYOUT='nchw')), ('nopolar', dict(WG0, SPHERE_POLAR=False)),
          ('nobwdsplit', dict(WG0, SPHERE_BWD_WEIGHT_SPLIT=False, SPHERE_BWD_DATA_SPLIT=False))]
SPHERE_CASES = [('sphere_%s_%s_%s' % (typ, mode, name), typ, mode, sw) for typ in ('Cassini', 'ERP') for mode in ('train', 'eval', 'train_t', 'eval_t')
                for name, sw in SPHERE if mode in ('train', 'eval') or name in ('wg0', 'wg200')]
MODELS = ('model_train', 'model_eval')
# the second fixture: (key, table type, mode, module switches, stride)
GRAD = [('scatter', dict(WG0, SPHERE_BWD_DATA='scatter')), ('nobwdt', dict(WG0, SPHERE_BWD_DATA_T=False)),
        ('bwwgather', dict(WG0, SPHERE_BWD_WEIGHT='gather'))]
GRAD_CASES = [('sphere_%s_train_%s' % (typ, name), typ, 'train', sw, 1) for typ in ('Cassini', 'ERP') for name, sw in GRAD] + \
             [('sphere_%s_train_s2' % typ, typ, 'train', WG0, 2) for typ in ('Cassini', 'ERP')]


def op_key(case):
  op, s, shape = case
  return '%s/s%d_%s' % (op, s, 'x'.join(str(v) for v in shape))


def all_keys():
  return ['%s/%s' % (sw, k) for sw in SWITCH_SETS for k in [op_key(c) for c in OPS] + [c[0] for c in SPHERE_CASES] + list(MODELS)]


def _rand(shape, seed, scale=1.0):
  return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32)).to(DEV)


# ------------------------------------------------------------------------------------------------ the spies
def _enc(a):
  if a is None:
    return '0'
  obj = getattr(a, '_obj', None)  # ctypes.byref(epilogue)
  if obj is not None:
    return ['E', int(obj.relu), int(bool(obj.add))] if hasattr(obj, 'relu') else 'P'
  if isinstance(a, ctypes.c_void_p):
    return 'P' if a.value else '0'
  if isinstance(a, float):
    return float(np.float32(a))
  return int(a)


class _LibSpy(object):

  def __init__(self, real, log):
    self._real, self._log = real, log

  def __getattr__(self, name):
    import mode_hip
    fn = getattr(self._real, name)
    launching = name in mode_hip.LAUNCHING and name != 'mode_debug_poison'  # (the stream is a launching entry's last parameter)
    if not launching and name != 'mode_weight_pack_reuse':
      return fn
    log = self._log

    def call(*args):
      log.append(['call', name, [_enc(a) for a in (args[:-1] if launching else args)]])
      return fn(*args)
    return call


class recording(object):
  """with recording(switches) as log: the module switches set, profiling on, the three spies in place; everything restored on exit."""

  def __init__(self, switches):
    self.switches = dict(switches)
    self.log = []

  def __enter__(self):
    from mode_hip import functional as HF, profiling
    self.prev = {k: getattr(HF, k) for k in list(self.switches) + ['lib', 'abs_max']}
    self.prev_region, self.prev_enabled = profiling.region, profiling.ENABLED
    for k, v in self.switches.items():
      setattr(HF, k, v)
    log, real_lib, real_abs_max, real_region = self.log, HF.lib, HF.abs_max, profiling.region
    HF.lib = lambda: _LibSpy(real_lib(), log)

    def abs_max(t):
      log.append(['amax', [int(v) for v in t.shape]])
      return real_abs_max(t)

    def region(name, nbytes=0, flops=0, device=None):
      log.append(['region', name, int(nbytes), int(flops)])
      return real_region(name, nbytes, flops, device)
    HF.abs_max = abs_max
    profiling.enable(True)
    profiling.region = region
    return log

  def __exit__(self, *exc):
    from mode_hip import functional as HF, profiling
    for k, v in self.prev.items():
      setattr(HF, k, v)
    profiling.region = self.prev_region
    profiling.enable(self.prev_enabled)
    return False


# ------------------------------------------------------------------------------------------------ the cases
def _bn(co, dims):
  bn = (torch.nn.BatchNorm3d if dims == 3 else torch.nn.BatchNorm2d)(co).to(DEV)
  with torch.no_grad():
    bn.weight.copy_(_rand((co,), 614).abs() + 0.5)
    bn.bias.copy_(_rand((co,), 615))
    bn.running_mean.copy_(_rand((co,), 616, 0.1))
    bn.running_var.copy_(_rand((co,), 617).abs() + 0.5)
  return bn


def run_op(case):
  """Runs the operator of `case` once (eval cases: twice) under the switches and spies as they stand."""
  from mode_hip import functional as HF
  op, s, shape = case
  o = lambda n: (n - 1) // s + 1
  if op.startswith('c3d_') or op.startswith('deconv'):
    B, ci, co, D, H, W = shape
    scale = (2.0 / (27 * ci))**0.5
    x = _rand((B, ci, D, H, W), 601)
    if op.startswith('deconv'):
      w = _rand((ci, co, 3, 3, 3), 602, scale)
      if op == 'deconv_fn':
        x.requires_grad_(True)
        w.requires_grad_(True)
        HF.deconv3d(x, w).backward(_rand((B, co, 2 * D, 2 * H, 2 * W), 604))
      else:
        bn, res = _bn(co, 3).eval(), _rand((B, co, 2 * D, 2 * H, 2 * W), 603)
        with torch.no_grad():
          HF.deconv3d_bn_eval(x, w, bn, add=res, relu=True)
          HF.deconv3d_bn_eval(x, w, bn, add=res, relu=True)
      return
    w = _rand((co, ci, 3, 3, 3), 602, scale)
    gy = _rand((B, co, o(D), o(H), o(W)), 604)
    if op == 'c3d_fwd':
      HF.conv3d_fwd(x, w, s)
    elif op == 'c3d_bwd_data':
      HF.conv3d_bwd_data(gy, w, x.shape, s)
    elif op == 'c3d_bwd_data_acc':
      HF.conv3d_bwd_data(gy, w, x.shape, s, acc=_rand((B, ci, D, H, W), 605))
    elif op == 'c3d_bwd_weight':
      HF.conv3d_bwd_weight(gy, x, s)
    elif op == 'c3d_bwd_weight_into':
      HF.conv3d_bwd_weight(gy, x, s, into=torch.zeros((co, ci, 3, 3, 3), device=DEV))
    elif op in ('c3d_fn_tagged', 'c3d_fn_untagged'):
      if op == 'c3d_fn_tagged':  # x out of a training BatchNorm pass: tagged with its maximum where the consumer's arithmetic wants one
        x.requires_grad_(True)
        x = HF.bn_act(_bn(ci, 3).train(), x, relu=True)
      else:
        x.requires_grad_(True)
      w.requires_grad_(True)
      HF.conv3d(x, w, s).backward(gy)
    elif op == 'c3d_eval':
      bn, res = _bn(co, 3).eval(), _rand(tuple(gy.shape), 603)
      with torch.no_grad():
        HF.conv3d_bn_eval(x, w, bn, s, add=res, relu=True)
        HF.conv3d_bn_eval(x, w, bn, s, add=res, relu=True)
    else:
      raise ValueError(op)
  elif op == 'cost_conv_eval':
    B, C, co, d4, H, W = shape
    ref, tgt, w = _rand((B, C, H, W), 601), _rand((B, C, H, W), 606), _rand((co, 2 * C, 3, 3, 3), 602, 0.05)
    bn = _bn(co, 3).eval()
    with torch.no_grad():
      HF.cost_conv_bn_eval(ref, tgt, w, d4, bn, relu=True)
  elif op.startswith('c2d_'):
    B, ci, co, H, W = shape
    dil = s
    x, w, gy = _rand((B, ci, H, W), 601), _rand((co, ci, 3, 3), 602, (2.0 / (9 * ci))**0.5), _rand((B, co, H, W), 604)
    if op == 'c2d_fwd':
      HF.conv2d_fwd(x, w, dil, f16=True)
    elif op == 'c2d_bwd_data_acc':
      HF.conv2d_bwd_data(gy, w, dil, acc=_rand((B, ci, H, W), 605))
    elif op == 'c2d_bwd_weight_into':
      HF.conv2d_bwd_weight(gy, x, dil, into=torch.zeros((co, ci, 3, 3), device=DEV))
    elif op == 'c2d_eval':
      bn, res = _bn(co, 2).eval(), _rand((B, co, H, W), 603)
      with torch.no_grad():
        HF.conv2d_bn_eval(x, w, bn, dil, add=res, relu=True)
        HF.conv2d_bn_eval(x, w, bn, dil, add=res, relu=True)
    else:
      raise ValueError(op)
  elif op == 'bn_act':
    y = _rand(shape, 601).requires_grad_(True)
    HF.bn_act(_bn(shape[1], len(shape) - 2).train(), y, relu=True).backward(_rand(shape, 604))
  elif op == 'classif':
    B, C, D, H, W = shape
    y = _rand(shape, 601).requires_grad_(True)
    conv = torch.nn.Conv3d(C, 1, 3, 1, 1, bias=False).to(DEV)
    HF.classif_head_train(y, _bn(C, 3).train(), conv).backward(_rand((B, 1, D, H, W), 604))
  else:
    raise ValueError(op)


def run_sphere(case, log):
  from models.basic.spherical_conv.sphere_conv import SphereConv, transposed_io
  key, typ, mode = case[:3]
  stride = case[4] if len(case) > 4 else 1
  torch.manual_seed(7)
  conv = SphereConv(128, 256, typ, 32, 32, 3, stride, 1).to(DEV)
  hw = (256, 128) if typ == 'Cassini' else (128, 256)
  t_ok = bool(conv.supports_transposed_io(1, torch.device(DEV)))
  log.append(['t_supported', t_ok])
  if mode.endswith('_t'):
    if not t_ok:
      return
    hw = hw[::-1]
  x = _rand((1, 32) + hw, 601)

  def go():
    if mode.startswith('train'):
      conv.train()
      x.requires_grad_(True)
      conv(x).backward(_rand((1, 32) + tuple((n - 1) // stride + 1 for n in hw), 604))
    else:
      bn = _bn(32, 2).eval()
      with torch.no_grad():
        conv.forward_bn(x, bn, add=_rand((1, 32) + hw, 603), relu=True)
        conv.forward_bn(x, bn, add=_rand((1, 32) + hw, 603), relu=True)
  if mode.endswith('_t'):
    with transposed_io():
      go()
  else:
    go()


def run_model(which):
  import models
  import recipe
  maxdisp, H, W, B = 16, 64, 32, 1
  net = models.ModeDisparity(maxdisp, 'Sphere', H, W, 'Cassini').to(DEV)
  net.load_state_dict(recipe.recipe_state_wc(recipe.load_manifest(), 31))
  left, right = [t.to(DEV) for t in recipe.recipe_images(B, H, W, 32)]
  if which == 'model_train':
    net.train()
    preds = net(left, right)
    sum((p * p).mean() for p in preds).backward()
  else:
    net.eval()
    with torch.no_grad():
      net(left, right)


def counts(log):
  c = collections.Counter(json.dumps(e) for e in log)
  return {k: c[k] for k in sorted(c)}


def record(sw, kind, case):
  """The events of one case under switch set `sw`: a list (operator and sphere cases) or counts per event (model cases)."""
  switches = dict(SWITCH_SETS[sw])
  if kind == 'sphere':
    switches.update(case[3])
  if kind == 'model':
    with recording(switches) as log:
      run_model(case)
    torch.cuda.synchronize()
    return counts(log)
  with recording(switches) as log:
    run_op(case) if kind == 'op' else run_sphere(case, log)
  torch.cuda.synchronize()
  return json.loads(json.dumps(log))


def jobs():
  for sw in SWITCH_SETS:
    for c in OPS:
      yield '%s/%s' % (sw, op_key(c)), sw, 'op', c
    for c in SPHERE_CASES:
      yield '%s/%s' % (sw, c[0]), sw, 'sphere', c
    for m in MODELS:
      yield '%s/%s' % (sw, m), sw, 'model', m


def grad_jobs():
  for sw in SWITCH_SETS:
    for c in GRAD_CASES:
      yield '%s/%s' % (sw, c[0]), sw, 'sphere', c


def main():
  grad = sys.argv[1:2] == ['sphere_grad']
  path = (sys.argv[2:] if grad else sys.argv[1:])[:1] or [OUT_GRAD if grad else OUT]
  out = {}
  for key, sw, kind, case in (grad_jobs() if grad else jobs()):
    out[key] = record(sw, kind, case)
    print(key, len(out[key]), flush=True)
  assert grad or sorted(out) == sorted(all_keys())
  with open(path[0], 'w') as f:
    f.write('{\n' + ',\n'.join('%s:%s' % (json.dumps(k), json.dumps(out[k], separators=(',', ':'))) for k in sorted(out)) + '\n}\n')  # a case per line


if __name__ == '__main__':
  main()
