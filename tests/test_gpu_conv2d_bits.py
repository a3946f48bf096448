"""GPU (-m gpu): the regular 3x3 Conv2d operators compute what they computed before csrc/conv2d.hip was split, bit for bit.

csrc/conv2d.hip became conv2d_f32_fwd.hip (the fp32 forward kernels, their launchers and the zero insertion), conv2d_f32_wgrad.hip
(the fp32 weight-gradient kernel, the split-K grid and the reduction) and conv2d.hip (the C entries of the whole 2-D family with one
argument check); the host code between an entry and its launches -- the tile choice, the split-K slices, the rows per work unit -- is
now written once.  The kernels' listings are unchanged (tools/isa_same.py); what a listing cannot show is whether the host still
launches them the same way, and the split-K partition decides the bits of a weight gradient.  tests/golden/conv2d_parent_bits.json
holds the SHA-256 of the operators' outputs at the commit before (tests/golden/make_golden_conv2d_bits.py, run once on the MI355X
there; its docstring derives which kernel instantiation and which S / run_groups each case reaches, and names the instantiations no
case reaches): the outputs are recomputed here on the same seeded inputs and their hashes compared, and each call is repeated once and
compared with torch.equal.  Every case asserts its route through HF._conv2d_route."""
import json
import os

import pytest
import torch

import make_golden_conv2d_bits as G

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(G.__file__)), 'conv2d_parent_bits.json')) as f:
  WANT = json.load(f)


def test_the_fixture_has_exactly_these_cases():
  assert sorted(WANT) == sorted(G.key(case) for case in G.CASES)


@pytest.mark.parametrize('case', G.CASES, ids=[G.key(case) for case in G.CASES])
def test_conv2d_bits_are_the_parents(case, monkeypatch):
  from mode_hip import functional as HF
  for name, value in G.settings(case).items():
    monkeypatch.setattr(HF, name, value)
  run = G.make(case)
  got = run()
  want = WANT[G.key(case)]
  assert list(got.shape) == want['shape']
  assert torch.isfinite(got).all()
  assert G.digest(got) == want['sha256'], '%s: the output differs from the parent commit\'s' % G.key(case)
  assert torch.equal(run(), got), 'not repeatable'
