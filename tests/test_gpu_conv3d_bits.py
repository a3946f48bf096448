"""GPU (-m gpu): the 3-D convolution operators compute what they computed before csrc/conv3d.hip was split, bit for bit.

csrc/conv3d.hip became conv3d_f32_fwd.hip (the fp32 forward kernels and their launchers), conv3d_f32_wgrad.hip (the fp32
weight-gradient kernels, their choice and the reduction) and conv3d.hip (the C entries of the whole 3-D family with their argument
checks); the host code between an entry and its launches -- the tile choice, the split-K slices, the depths per work unit -- is now
written once.  The kernels' listings are unchanged (tools/isa_same.py); what a listing cannot show is whether the host still launches
them the same way, and the split-K partition decides the bits of a weight gradient.  tests/golden/conv3d_parent_bits.json holds the
SHA-256 of the operators' outputs at the commit before (tests/golden/make_golden_conv3d_bits.py, run once on the MI355X there; its
docstring says which kernel instantiation each case reaches and why): the outputs are recomputed here on the same seeded inputs and
their hashes compared, and each call is repeated once and compared with torch.equal.

Not reached by any case: conv3d_bwd_weight_kernel<S, WTH>, the fallback for samples of 2^29 elements and more -- no test of a few
seconds gets there; the listing comparison alone covers it."""
import json
import os

import pytest
import torch

import make_golden_conv3d_bits as G

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(G.__file__)), 'conv3d_parent_bits.json')) as f:
  WANT = json.load(f)


def test_the_fixture_has_exactly_these_cases():
  assert sorted(WANT) == sorted(G.key(case) for case in G.CASES)


@pytest.mark.parametrize('case', G.CASES, ids=[G.key(case) for case in G.CASES])
def test_conv3d_bits_are_the_parents(case, monkeypatch):
  from mode_hip import functional as HF
  monkeypatch.setattr(HF, 'CONV_ARITH', case[1])
  monkeypatch.setattr(HF, 'CONV3D_S1_F16', case[2])
  run = G.make(case)
  got = run()
  want = WANT[G.key(case)]
  assert list(got.shape) == want['shape']
  assert torch.isfinite(got).all()
  assert G.digest(got) == want['sha256'], '%s: the output differs from the parent commit\'s' % G.key(case)
  assert torch.equal(run(), got), 'not repeatable'
