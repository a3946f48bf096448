#!/usr/bin/env python3
"""tests/golden/augment_lighting.npz: the reference's Lighting(0.1, eigval, eigvec) (dataloader/preprocess.py:78-95) run under a seed.

  python tests/golden/make_golden_augment.py [path/to/reference]

Development container only (needs the reference checkout); the tests read the committed .npz.  The reference file is loaded by path
(importlib.util.spec_from_file_location): the package's __init__ needs cv2 and is not imported.  Harness stand-in (it lives only in
this script, no reference file is edited or copied): an empty module registered as `torchvision` and `torchvision.transforms` -- the
file imports the name at its top and uses it only inside functions that are not called here.

Stored: the float32 input image (3, 5, 7), the three alphas (re-drawn under the same seed: Lighting's only draw is
img.new().resize_(3).normal_(0, alphastd), the first draw after the seed), the reference's eigval / eigvec, its output, and
shift = output - input evaluated per channel on a zero image (so it is the reference's own `rgb`, bit for bit).  The script asserts that
input + shift reproduces the output bit for bit."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))
SEED, ALPHASTD = 20221, 0.1


def load_reference_preprocess():
  stub = types.ModuleType('torchvision')
  stub.transforms = types.ModuleType('torchvision.transforms')
  sys.modules.setdefault('torchvision', stub)
  sys.modules.setdefault('torchvision.transforms', stub.transforms)
  spec = importlib.util.spec_from_file_location('reference_preprocess', os.path.join(REF, 'dataloader', 'preprocess.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def main():
  ref = load_reference_preprocess()
  pca = getattr(ref, '__imagenet_pca')
  eigval, eigvec = pca['eigval'], pca['eigvec']
  light = ref.Lighting(ALPHASTD, eigval, eigvec)
  img = torch.from_numpy(np.random.RandomState(7).rand(3, 5, 7).astype(np.float32))
  torch.manual_seed(SEED)
  out = light(img)
  torch.manual_seed(SEED)
  shift = light(torch.zeros(3, 1, 1))[:, 0, 0]  # 0 + rgb = rgb
  torch.manual_seed(SEED)
  alpha = torch.empty(0).resize_(3).normal_(0, ALPHASTD)
  assert torch.equal(img + shift.view(3, 1, 1), out)
  path = os.path.join(HERE, 'augment_lighting.npz')
  np.savez(path, img=img.numpy(), alpha=alpha.numpy(), shift=shift.numpy(), eigval=eigval.numpy(), eigvec=eigvec.numpy(), out=out.numpy(),
           alphastd=np.float32(ALPHASTD), seed=np.int64(SEED))
  print('wrote', path, os.path.getsize(path), 'bytes; shift', shift.tolist())


if __name__ == '__main__':
  main()
