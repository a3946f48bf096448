"""GPU (-m gpu): every layer still runs on the C entry it ran on before functional.py decided each family's kernel route in one place,
with the same arguments, the same maximum passes and the same profiling labels and byte counts.

mode_hip.functional used to restate "split kernel at this size? stride 2? fp16 pieces?" at every call site; now _conv3d_route,
_conv2d_route and _sphere_fwd_route answer once per family and the sites ask them.  That is host code only, so the outputs' bits are
pinned already (tests/test_gpu_conv3d_bits.py, tests/test_gpu_sphere_win_bits.py); what they do not see is a route that changed under
a switch set no bit test runs.  tests/golden/routes_parent.json holds the trace of the commit before (tests/golden/make_golden_routes.py,
run once on the MI355X there; its docstring describes the events and the cases): the cases are replayed here through the same spies on
functional.lib, functional.abs_max and profiling.region -- names the rewritten code must still resolve at call time -- and compared:
operator and sphere cases as sequences, the two model cases as counts per event.

tests/golden/routes_parent_sphere_grad.json is a second trace, recorded later: at the commit before the spherical GRADIENTS got their
route functions (_sphere_bwd_data_route, _sphere_bwd_data_t_route, _sphere_bwd_weight_route) and the plans became records, with the
recorder's second case list (GRAD_CASES) run against that commit's functional.py.  The first trace sets none of the gradient switches;
this one runs the SphereConv training step under SPHERE_BWD_DATA = 'scatter', SPHERE_BWD_DATA_T = False and SPHERE_BWD_WEIGHT =
'gather', and one stride-2 layer, on both table types.  routes_parent.json itself is the file recorded for the first change, unchanged."""
import json
import os

import pytest

import make_golden_routes as G

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(G.__file__)), 'routes_parent.json')) as f:
  WANT = json.load(f)

with open(G.OUT_GRAD) as f:
  WANT_GRAD = json.load(f)

JOBS = list(G.jobs())
GRAD_JOBS = list(G.grad_jobs())


def test_the_fixture_has_exactly_these_cases():
  assert sorted(WANT) == sorted(G.all_keys()) == sorted(j[0] for j in JOBS)
  assert sorted(WANT_GRAD) == sorted(j[0] for j in GRAD_JOBS) and len(GRAD_JOBS) == 24


@pytest.mark.parametrize('key,sw,kind,case', JOBS, ids=[j[0] for j in JOBS])
def test_routes_are_the_parents(key, sw, kind, case):
  got, want = G.record(sw, kind, case), WANT[key]
  if kind == 'model':
    diff = {k: (want.get(k, 0), got.get(k, 0)) for k in set(want) | set(got) if want.get(k, 0) != got.get(k, 0)}
    assert not diff, '%s: (parent count, count now) per event that differs: %s' % (key, diff)
  else:
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, '%s: event %d differs: parent %s, now %s' % (key, first, want[first:first + 1], got[first:first + 1])


@pytest.mark.parametrize('key,sw,kind,case', GRAD_JOBS, ids=[j[0] for j in GRAD_JOBS])
def test_sphere_gradient_routes_are_the_parents(key, sw, kind, case):
  got, want = G.record(sw, kind, case), WANT_GRAD[key]
  first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
  assert got == want, '%s: event %d differs: parent %s, now %s' % (key, first, want[first:first + 1], got[first:first + 1])
