#!/usr/bin/env python3
"""Golden vectors for utils.evaluation and the SILog loss, made by the REFERENCE's utils/evaluation.py on CPU torch in the dev container.

  python tests/golden/make_golden_metrics.py     # writes metrics.npz and script_imports.json

metrics.npz: the inputs of each case (`<case>/pred`, `<case>/gt`, fp32), and for every call of a reference metric function its
result (`val/<i>`) with the result's type, or the name of the exception it raised (`calls`, JSON).  The loss truth is
oracle.fusion_ref.silog_loss (train_fusion.py:82-87 restated), stored as the reference's own fp32 value (`loss/<case>`).
script_imports.json: every `from models|utils|dataloader... import ...` of the reference's top-level scripts (an ast scan: module,
names, script and line; no source text) and the signatures of the reference's evaluation functions.

The reference file imports torch only; it is loaded by path (its `utils` package would shadow ours)."""
import ast
import importlib.util
import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import fusion_ref  # noqa: E402

REF = '/root/reference'
EVAL_FUNCS = ['mae', 'max_ae', 'rmse', 'absrel', 'sqrel', 'silog', 'pixel_error_pct', 'D1', 'delta_acc', 'threshold_acc']
# (function, leading threshold arguments): every function, the thresholds of the reference's scripts and the fp32-rounding corners
CALLS = [('mae', ()), ('max_ae', ()), ('rmse', ()), ('absrel', ()), ('sqrel', ()), ('silog', ()),
         ('pixel_error_pct', (0.7,)), ('pixel_error_pct', (1,)), ('pixel_error_pct', (3,)), ('pixel_error_pct', (5,)),
         ('D1', (3, 0.05)), ('D1', (0.5, 0.05)), ('D1', (0.7, 0.1)),
         ('delta_acc', (1,)), ('delta_acc', (2,)), ('delta_acc', (3,)),
         ('threshold_acc', (0.25,)), ('threshold_acc', (0.3,)), ('threshold_acc', (0.1,))]


def load_reference_evaluation():
  spec = importlib.util.spec_from_file_location('ref_evaluation', os.path.join(REF, 'utils', 'evaluation.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def _exact_pairs(g, t):
  """(pred, gt) with pred - gt == t EXACTLY in fp32, from the candidates g (fp32)."""
  p = (g + t).astype(np.float32)
  keep = (p - g).astype(np.float32) == t
  return p[keep], g[keep]


def _check_corners(p, g):
  """Each fp32 rule changes a count of the boundary case: a kernel that compared or multiplied in double would miss it."""
  with np.errstate(all='ignore'):
    e32 = np.abs((p - g).astype(np.float32))
    e64 = e32.astype(np.float64)
    assert (e32 >= np.float32(0.7)).sum() != (e64 >= 0.7).sum()  # pixel_error_pct(0.7): the threshold cast to fp32
    g64 = g.astype(np.float64)
    for tp, tc in ((0.5, 0.05), (0.7, 0.1)):  # D1: th_pct * g as an fp32 product, not in double
      d1_32 = ((e32 >= np.float32(tp)) & (e32 >= (np.float32(tc) * g).astype(np.float32))).sum()
      assert d1_32 != ((e32 >= np.float32(tp)) & (e64 >= np.float64(np.float32(tc)) * g64)).sum()
    r = np.maximum((p / g).astype(np.float32), (g / p).astype(np.float32))
    assert (r < np.float32(1.3)).sum() != (r.astype(np.float64) < 1.3).sum()  # threshold_acc(0.3): the bound rounded to fp32
    assert (r == np.float32(1.25)).any() and not (r < np.float32(1.25))[r == np.float32(1.25)].any()  # ratio exactly 1.25


def cases():
  rs = np.random.RandomState(2024)
  out = {}
  # finite positive data: every mean is a number (gt in (0.5, 60), pred a noisy copy)
  g = (0.5 + 59.5 * rs.rand(3001)).astype(np.float32)
  out['finite'] = ((g * (1 + 0.2 * rs.randn(3001))).astype(np.float32), g)
  # random data with NaN, +-inf, zeros and negatives in both maps
  p = (rs.randn(4099) * 20 + 10).astype(np.float32)
  g = (rs.randn(4099) * 20 + 10).astype(np.float32)
  for arr in (p, g):
    idx = rs.choice(4099, 60, replace=False)
    arr[idx[:15]] = np.nan
    arr[idx[15:25]] = np.inf
    arr[idx[25:35]] = -np.inf
    arr[idx[35:60]] = 0
  out['specials'] = (p, g)
  # the same random data without NaN / inf (zeros and negatives kept): the sums stay finite
  p2, g2 = (rs.randn(2053) * 20 + 10).astype(np.float32), (rs.randn(2053) * 20 + 10).astype(np.float32)
  p2[rs.choice(2053, 30, replace=False)] = 0
  g2[rs.choice(2053, 30, replace=False)] = 0
  out['signed'] = (p2, g2)
  # threshold corners: |d| = float32(0.7) (>= 0.7 holds in fp32 although float32(0.7) < 0.7), |d| = float32(0.05) * g in fp32 (D1's
  # product), |d| = 3 with 3 >= 0.05 g and below; ratios exactly 1.25, 1.5625, 1.953125 (not < bound) and float32(1.3) (threshold_acc(0.3))
  cand = (1 + 40 * rs.rand(400)).astype(np.float32)
  # |d| = float32(0.7) exactly: g in [0.5, 1) (above 1 the sum g + 0.7f is never exact) and p = 0.7f with g = 0
  pa, ga = _exact_pairs((0.5 + 0.5 * rs.rand(200)).astype(np.float32), np.float32(0.7))
  pa, ga = np.concatenate([pa, [np.float32(0.7)]]).astype(np.float32), np.concatenate([ga, [0]]).astype(np.float32)
  assert pa.size >= 20 and (np.abs(pa - ga) == np.float32(0.7)).all()
  tb = (np.float32(0.05) * cand).astype(np.float32)
  pb = (cand + tb).astype(np.float32)
  kb = (pb - cand).astype(np.float32) == tb
  pb, gb = pb[kb], cand[kb]
  tc = (np.float32(0.1) * cand).astype(np.float32)
  pc = (cand - tc).astype(np.float32)
  kc = (cand - pc).astype(np.float32) == tc
  pc, gc = pc[kc], cand[kc]
  assert pb.size >= 5 and pc.size >= 5
  pd, gd = _exact_pairs(np.array([10, 40, 60, 61, 59.5], np.float32), np.float32(3))
  ratio_g = np.array([4, 8, 64, 5, 16, 256, 1, 2], np.float32)
  ratio_p = np.array([5, 10, 80, 4, 25, 500, np.float32(1.3), np.float32(2) * np.float32(1.3)], np.float32)
  out['boundary'] = (np.concatenate([pa, pb, pc, pd, ratio_p]).astype(np.float32),
                     np.concatenate([ga, gb, gc, gd, ratio_g]).astype(np.float32))
  _check_corners(*out['boundary'])
  # gt = 0 with pred > 0 (ratio inf), pred = gt = 0 (0 / 0 = NaN), gt > 0 with pred = 0, negative gt, pred < 0
  out['zeros'] = (np.array([1, 2.5, 0, 0, 0, 3, -1, 2, 0.5, 7], np.float32), np.array([0, 0, 0, 0, 2, -3, 2, 2, 0.25, 7], np.float32))
  out['empty'] = (np.zeros(0, np.float32), np.zeros(0, np.float32))
  return out


def script_imports():
  rows = []
  for name in sorted(os.listdir(REF)):
    if not name.endswith('.py'):
      continue
    tree = ast.parse(open(os.path.join(REF, name)).read())
    for node in tree.body:
      if isinstance(node, ast.ImportFrom) and node.module and node.module.split('.')[0] in ('models', 'utils', 'dataloader'):
        rows.append({'script': name, 'line': node.lineno, 'module': node.module, 'names': [a.name for a in node.names]})
  return rows


def main():
  ev = load_reference_evaluation()
  arrays, calls = {}, []
  for case, (p, g) in cases().items():
    arrays[case + '/pred'], arrays[case + '/gt'] = p, g
    tp, tg = torch.from_numpy(p), torch.from_numpy(g)
    for fn, args in CALLS:
      rec = {'case': case, 'fn': fn, 'args': list(args)}
      try:
        v = getattr(ev, fn)(*args, tp, tg)
      except Exception as e:  # noqa: BLE001 -- the exception's name is the golden value
        rec['raises'] = type(e).__name__
      else:
        rec['type'] = type(v).__name__
        if isinstance(v, np.ndarray):
          rec['dtype'], rec['shape'] = str(v.dtype), list(v.shape)
        key = 'val/%d' % len(calls)
        arrays[key] = np.asarray(v, dtype=np.float64 if isinstance(v, float) else v.dtype)
        rec['key'] = key
      calls.append(rec)
    with torch.no_grad():
      arrays['loss/' + case] = np.asarray(fusion_ref.silog_loss(0.5, tp, tg).numpy(), np.float32)
  arrays['calls'] = np.array(json.dumps(calls))
  np.savez_compressed(os.path.join(HERE, 'metrics.npz'), **arrays)
  sigs = {}
  for fn in EVAL_FUNCS:
    sig = inspect.signature(getattr(ev, fn))
    sigs[fn] = [[k, None if prm.default is inspect.Parameter.empty else repr(prm.default)] for k, prm in sig.parameters.items()]
  with open(os.path.join(HERE, 'script_imports.json'), 'w') as f:
    json.dump({'imports': script_imports(), 'evaluation_signatures': sigs}, f, indent=1)
    f.write('\n')
  print('wrote metrics.npz (%d calls) and script_imports.json' % len(calls))


if __name__ == '__main__':
  main()
