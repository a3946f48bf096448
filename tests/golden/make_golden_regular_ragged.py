#!/usr/bin/env python3
"""Golden vectors for ModeDisparity(conv='Regular') at a RAGGED size: 288 x 544, whose quarter-resolution plane 72 x 136 is no
multiple of 64 (or of 16) in either axis -- the SPP pyramid pools 9 x 17 blocks at k = 8 against 4 x 8 at k = 16, 2 x 4 at k = 32 and
1 x 2 at k = 64, with rows and columns that belong to no block.  Made by the imported reference like make_golden_regular.py.

  python tests/golden/make_golden_regular_ragged.py      # writes model_regular_ragged.npz

The fp64 "truth" is the reference itself evaluated in float64."""
import json
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import make_golden as mg
from make_golden import HERE, recipe

CFG = dict(maxdisp=16, H=288, W=544, B=2, seed=310)


def main():
  torch.set_num_threads(8)
  models, _ = mg.import_reference()
  c = CFG
  torch.manual_seed(0)
  m = models.ModeDisparity(c['maxdisp'], 'Regular')
  manifest = mg.load_recipe(m, c['seed'])
  left, right = recipe.recipe_images(c['B'], c['H'], c['W'], c['seed'] + 1)
  gt = recipe.recipe_disparity(c['B'], c['H'], c['W'], c['seed'] + 2, c['maxdisp'])
  mask = ~torch.isnan(gt)
  out = dict(cfg=np.array([c['maxdisp'], c['H'], c['W'], c['B'], c['seed']]), manifest=np.array(json.dumps([[k, list(s)] for k, s in manifest])))
  sub = (slice(None), slice(None), slice(None, None, 4), slice(None, None, 4))
  m.train()
  preds = m(left, right)
  loss = 0.5 * F.smooth_l1_loss(preds[0][mask], gt[mask]) + 0.7 * F.smooth_l1_loss(preds[1][mask], gt[mask]) + F.smooth_l1_loss(preds[2][mask], gt[mask])
  loss.backward()
  out['train/loss'] = np.array(float(loss))
  for i, p in enumerate(preds):
    out['train/pred%d' % (i + 1)] = p.detach()[sub].numpy()
  out.update({'train/' + k: v for k, v in mg.grad_summary(m).items()})
  bns = [x for x in m.modules() if isinstance(x, (nn.BatchNorm2d, nn.BatchNorm3d))]
  for x in bns:
    x.momentum = 1.0
  with torch.no_grad():
    m(left, right)
  for x in bns:
    x.momentum = 0.1
  out.update(mg.bn_stats(m))
  m.eval()
  with torch.no_grad():
    out['eval/pred3'] = m(left, right)[sub].numpy()
  # float64 evaluation by the reference itself (torch.FloatTensor pointed at the double type for the cost volume, as in
  # make_golden_regular.py)
  m64 = models.ModeDisparity(c['maxdisp'], 'Regular').double()
  m64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in recipe.recipe_state(manifest, c['seed']).items()})
  float_tensor = torch.FloatTensor
  torch.FloatTensor = torch.DoubleTensor
  m64.train()
  with torch.no_grad():
    t = m64(left.double(), right.double())
  for i, p in enumerate(t):
    out['truth64/train_pred%d' % (i + 1)] = p[sub].numpy()
  sd = m64.state_dict()
  for k, v in out.items():
    if k.startswith('bn/'):
      sd[k[3:]] = torch.from_numpy(v).double()
  m64.load_state_dict(sd)
  m64.eval()
  with torch.no_grad():
    out['truth64/eval_pred3'] = m64(left.double(), right.double())[sub].numpy()
  torch.FloatTensor = float_tensor
  np.savez_compressed(os.path.join(HERE, 'model_regular_ragged.npz'), **out)
  print('wrote model_regular_ragged.npz: loss %.5f; E_ref train %.2e eval %.2e' %
        (float(loss), max(np.abs(out['train/pred%d' % i] - out['truth64/train_pred%d' % i]).max() for i in (1, 2, 3)),
         np.abs(out['eval/pred3'] - out['truth64/eval_pred3']).max()))


if __name__ == '__main__':
  main()
