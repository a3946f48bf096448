"""CPU: the host code of the regular 3x3 Conv2d family answers what it answered before csrc/conv2d.hip was split (no launch).

tests/golden/conv2d_parent_host.json was recorded from a build of the commit before (tests/golden/make_golden_conv2d_host.py; its
docstring lists the grid and the calls): the four query functions whose bodies moved, bit for bit, and the return code of calls that
are wrong in exactly one way, over the family's twelve compute entries and mode_zero_insert2.  The one argument check of conv2d.hip
examines sizes, then the dilation, then the size rule of the kernel the entry launches, then pointers, then what concerns the entry
alone; a call that is wrong in two ways may therefore be refused for the other reason than before, and none is here."""
import json
import os

import pytest

import mode_hip
import make_golden_conv2d_host as G

with open(os.path.join(os.path.dirname(os.path.abspath(G.__file__)), 'conv2d_parent_host.json')) as f:
  WANT = json.load(f)

CASES = G.refusal_cases()


def test_the_fixture_has_exactly_these_cases():
  assert sorted(WANT['refusals']) == sorted(case[0] for case in CASES)
  assert {case[1] for case in CASES} == set(G.ENTRIES) | {'mode_zero_insert2'}
  declared = {n for n in mode_hip.SIGNATURES if n.startswith('mode_conv2d_') and not n.endswith(('_bytes', '_supported'))}
  assert declared == set(G.ENTRIES), 'an entry of the family without refusal cases'


@pytest.mark.parametrize('name', sorted(WANT['queries']))
def test_queries_answer_as_the_parent(name):
  got, want = G.queries(mode_hip.lib())[name], WANT['queries'][name]
  assert len(got) == len(want)
  assert got == want, [i for i in range(len(want)) if got[i] != want[i]][:8]


@pytest.mark.parametrize('case', CASES, ids=[case[0] for case in CASES])
def test_a_single_fault_is_refused_with_the_parents_code(case):
  rc, message = G.call(mode_hip.lib(), case)
  assert rc == WANT['refusals'][case[0]] and rc in (-1, -2)
  assert case[1].encode() in message, message
