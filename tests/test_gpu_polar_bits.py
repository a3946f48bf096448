"""GPU (-m gpu): the two polar kernels of the spherical gradients compute what they computed before they were rescheduled, bit for bit.

sphere_bwd_data_adj9_kernel (csrc/sphere_conv.hip) went from 4 to 8 waves per 64-pixel tile and sphere_bww_polar_split_kernel
(csrc/sphere_win_bww.hip) issues an item's loads in one batch ahead of its barrier; neither change touches the sequence of operations
behind an output element.  tests/golden/polar_parent_bits.json holds the SHA-256 of the operators' outputs at the commit before
(tests/golden/make_golden_polar_bits.py, run once on the MI355X there): the outputs are recomputed here on the same seeded inputs and
their hashes compared, and each call is repeated once and compared with torch.equal."""
import json
import os

import pytest
import torch

import make_golden_polar_bits as G
from mode_hip import functional as HF

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(G.__file__)), 'polar_parent_bits.json')) as f:
  WANT = json.load(f)


@pytest.fixture(autouse=True)
def _default_arithmetic():
  HF.set_conv_arith('bf16x6')
  yield
  HF.set_conv_arith('bf16x6')


def _check(kind, make, case):
  run = make(case)
  got = run()
  want = WANT[G.key(kind, case)]
  assert list(got.shape) == want['shape']
  assert torch.isfinite(got).all()
  assert G.digest(got) == want['sha256'], '%s: the output differs from the parent commit\'s' % G.key(kind, case)
  assert torch.equal(run(), got), 'not repeatable'


@pytest.mark.parametrize('case', G.BWD_DATA, ids=lambda c: G.key('bwd_data', c))
def test_sphere_input_gradient_bits_are_the_parents(case):
  _check('bwd_data', G.bwd_data, case)


@pytest.mark.parametrize('case', G.BWD_WEIGHT, ids=lambda c: G.key('bwd_weight', c))
def test_sphere_weight_gradient_bits_are_the_parents(case):
  _check('bwd_weight', G.bwd_weight, case)
