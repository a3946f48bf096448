"""GPU (-m gpu): the windowed spherical kernels compute what they computed before their source was split, bit for bit.

csrc/sphere_conv_win.hip became one file per pass (sphere_win_fwd.hip, sphere_win_bww.hip, sphere_win_bwd_data.hip) around
csrc/sphere_win_internal.h; a move changes no instruction.  tests/golden/sphere_win_parent_bits.json holds the SHA-256 of the
operators' outputs at the commit before (tests/golden/make_golden_sphere_win_bits.py, run once on the MI355X there): the outputs are
recomputed here on the same seeded inputs and their hashes compared, and each call is repeated once and compared with torch.equal.
tests/test_sphere_win_bits_plan.py shows on the host that the cases' table reaches every kernel class."""
import json
import os

import pytest
import torch

import make_golden_sphere_win_bits as G

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(G.__file__)), 'sphere_win_parent_bits.json')) as f:
  WANT = json.load(f)

CASES = [(kind, make, case) for kind, make, cases in G.KINDS for case in cases]


def test_the_fixture_has_exactly_these_cases():
  assert sorted(WANT) == sorted(G.key(kind, case) for kind, _, case in CASES)


@pytest.mark.parametrize('kind,make,case', CASES, ids=[G.key(kind, case) for kind, _, case in CASES])
def test_sphere_win_bits_are_the_parents(kind, make, case):
  run = make(case)
  got = run()
  want = WANT[G.key(kind, case)]
  assert list(got.shape) == want['shape']
  assert torch.isfinite(got).all()
  assert G.digest(got) == want['sha256'], '%s: the output differs from the parent commit\'s' % G.key(kind, case)
  assert torch.equal(run(), got), 'not repeatable'
