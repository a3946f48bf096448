"""CPU tier: the guard-band harness (tests/guard_bands.py) can fail, and the GPU operator table covers the whole launching C-ABI.

A deliberately broken kernel cannot be run on a shared GPU, so this file is the evidence that tests/test_gpu_guard_bands.py would
notice a wrong one: on CPU tensors, writes one element outside a guarded buffer are reported with allocation, side and offsets; a
write equal to one fill's pattern is caught under the other fill; an operator that reads one element past its input -- and multiplies
it by zero -- breaks finiteness or bit equality; a well-behaved operator passes; buffers made inside a Function.backward are guarded.
The allocations below are made from this file, which stands in for the host code (only_from=THIS)."""
import os

import pytest
import torch

import guard_bands as GB
import mode_hip

THIS = os.path.abspath(__file__)
HERE = os.path.dirname(THIS)


def _raw(t, first_byte, n):
  """n bytes of t's underlying storage starting first_byte bytes after t's first element (negative: before it)."""
  st = t.untyped_storage()
  whole = torch.empty(0, dtype=torch.uint8).set_(st, 0, (st.nbytes(),))
  at = t.storage_offset() * t.element_size() + first_byte
  return whole[at:at + n]


def test_views_are_aligned_contiguous_and_keep_their_content():
  with GB.guarded(0, only_from=(THIS,)) as gb:
    a = torch.empty(3, 5)
    b = torch.zeros(7, dtype=torch.int64)
    c = torch.ones(3, dtype=torch.bfloat16)
    d = torch.full((2, 2), 3.0)
    e = a.new_zeros(4)
    f = a.new_empty(6)
    g = torch.empty_like(a.t())
    src = torch.arange(15.0).view(3, 5)  # (arange: torch's own operator, not intercepted)
    h = src.clone()
    i = src.t().contiguous()
    j = torch.zeros_like(b)
    k = GB.place(torch.arange(5, dtype=torch.int32))
    assert len(gb.allocations) == 11, [x.describe() for x in gb.allocations]
    for t in (a, b, c, d, e, f, h, i, j, k):
      assert t.is_contiguous() and t.data_ptr() % 256 == 0
    assert g.stride() == (1, 5)
    assert torch.isnan(a).all() and torch.isnan(f).all()  # an "empty" buffer carries the float pattern
    assert not b.any() and not e.any() and not j.any() and bool((c == 1).all()) and bool((d == 3).all())
    assert torch.equal(h, src) and torch.equal(i, src.t()) and k.tolist() == [0, 1, 2, 3, 4]
    for al, nbytes in zip(gb.allocations, (60, 56, 6, 16, 16, 24, 60, 60, 60, 56, 20)):
      assert al.nbytes == nbytes and al.front == 256 * 1024 and al.rear_at == al.front + (nbytes + 3) // 4 * 4
      assert al.block.numel() == al.rear_at + al.front
    assert gb.allocations[0].where == 'tests/test_guard_bands_host.py:%d' % (test_views_are_aligned_contiguous_and_keep_their_content.__code__.co_firstlineno + 2)
    assert gb.allocations[-1].kind == 'placed'
    GB.check()
  with GB.guarded(1, only_from=(THIS,)):
    big = torch.empty(100000, dtype=torch.float64)  # guard = the tensor's own bytes once those exceed 256 KiB
    al = GB.current().allocations[0]
    assert al.front == 800000 and big.data_ptr() % 256 == 0 and bool((big == 1.0).all())
    assert _raw(torch.empty(4), -4, 4).view(torch.int32).item() == 0x3f803f80
    assert _raw(torch.zeros(4, dtype=torch.int32), 16, 4).view(torch.int32).item() == 2
    assert _raw(torch.zeros(3, dtype=torch.uint8), 3, 1).item() == 2  # the pad up to 4 bytes carries the pattern


def test_allocations_from_other_files_are_left_alone():
  with GB.guarded(0) as gb:  # the default: only the package's files
    t = torch.zeros(5)
    assert not gb.allocations and t.data_ptr() != 0


@pytest.mark.parametrize('fill', [0, 1])
def test_a_write_past_either_end_is_reported_with_allocation_side_and_offsets(fill):
  with GB.guarded(fill, only_from=(THIS,)):
    quiet = torch.zeros(9)
    out = torch.zeros(3, 5)
    line = test_a_write_past_either_end_is_reported_with_allocation_side_and_offsets.__code__.co_firstlineno + 4
    GB.check()
    _raw(out, 60, 4).view(torch.int32)[0] = 0x12345678  # one element past the end (no byte of it equals either pattern's)
    with pytest.raises(GB.GuardError) as ei:
      GB.check()
    (al, side, first, last), = ei.value.reports
    assert (al.where, al.shape, side) == ('tests/test_guard_bands_host.py:%d' % line, (3, 5), 'rear')
    assert (first, last) == (60, 63)
    _raw(out, -4, 4).view(torch.int32)[0] = 0x12345678  # one element before the start
    with pytest.raises(GB.GuardError) as ei:
      GB.check()
    sides = {r[1]: r[2:] for r in ei.value.reports}
    assert set(sides) == {'front', 'rear'} and sides['front'] == (-4, -1) and sides['rear'] == (60, 63)
    assert 'test_guard_bands_host.py:%d (3, 5) float32 (60 bytes): front guard damaged' % line in str(ei.value)
    assert quiet.sum() == 0


def test_byte_offsets_of_a_longer_overrun_and_of_a_narrow_dtype():
  with GB.guarded(0, only_from=(THIS,)):
    t = torch.zeros(5, dtype=torch.uint8)  # 5 bytes: 3 pad bytes, then the rear guard
    _raw(t, 5, 1)[0] = 0xff  # first byte past the end lies in the pad
    _raw(t, 100, 28).fill_(0xff)
    with pytest.raises(GB.GuardError) as ei:
      GB.check()
    (al, side, first, last), = ei.value.reports
    assert (side, first, last, al.nbytes) == ('rear', 5, 127, 5)
    w = torch.zeros(4, dtype=torch.int64)
    _raw(w, -256 * 1024, 8).view(torch.int64)[0] = 0  # the far end of the front guard
    with pytest.raises(GB.GuardError) as ei:
      GB.check()
    rep = [r for r in ei.value.reports if r[0].shape == (4,)]
    assert len(rep) == 1 and rep[0][1:] == ('front', -256 * 1024, -256 * 1024)  # the int64 pattern 1: only its low byte changed


def test_a_write_equal_to_one_fills_pattern_is_caught_by_the_other():
  def op():
    out = torch.zeros(6)
    _raw(out, 24, 4).view(torch.int32)[0] = 0x7fc00000  # past the end: exactly the first fill's pattern
    return out
  with GB.guarded(0, only_from=(THIS,)):
    op()
    GB.check()  # invisible here ...
  with GB.guarded(1, only_from=(THIS,)):
    op()
    with pytest.raises(GB.GuardError):
      GB.check()
  with pytest.raises(GB.GuardError) as ei:  # ... so under_two_fills, which runs both, reports it
    GB.under_two_fills(op, only_from=(THIS,))
  assert ei.value.reports[0][1:] == ('rear', 24, 27)


def _reads_one_past(x):
  """A fake operator: y[i] = x[i] + 0 * x[i + 1] -- the last output fetches the element behind x and multiplies it by zero."""
  shifted = x.as_strided(x.shape, x.stride(), x.storage_offset() + 1)
  return x + 0.0 * shifted


def test_an_over_read_multiplied_by_zero_breaks_finiteness_or_bit_equality():
  def case():
    x = GB.place(torch.arange(8.0))
    return _reads_one_past(x)
  with pytest.raises(AssertionError, match='non-finite values although every input is finite'):
    GB.under_two_fills(case, only_from=(THIS,))

  def case_int():  # integers: no NaN; the two fills give different values
    x = GB.place(torch.arange(8))
    return x + x.as_strided(x.shape, x.stride(), x.storage_offset() + 1)
  with pytest.raises(AssertionError, match=r'out \(8,\) differs between the two guard fills in 1 of 8 elements \(first flat index 7'):
    GB.under_two_fills(case_int, only_from=(THIS,))

  def case_front():  # one element BEFORE the input, added: finite under the second fill only, and different
    x = GB.place(torch.arange(8.0))
    y = torch.empty(8)
    torch.add(x, x.as_strided(x.shape, x.stride(), x.storage_offset() - 1), out=y)
    return y
  with pytest.raises(AssertionError):
    GB.under_two_fills(case_front, only_from=(THIS,))


def test_reading_an_unwritten_workspace_shows_too():
  def case():
    x = GB.place(torch.arange(4.0))
    ws = torch.empty(4)
    return x + 0.0 * ws
  with pytest.raises(AssertionError, match='non-finite'):
    GB.under_two_fills(case, only_from=(THIS,))


def test_a_well_behaved_operator_passes():
  def case():
    x = GB.place(torch.arange(12.0).view(3, 4))
    ws = torch.empty(3, 4)
    torch.mul(x, 2.0, out=ws)
    out = torch.zeros_like(x)
    out += ws
    return {'y': out, 'parts': [out.sum(), 2.5], 'idx': torch.argmax(out)}
  out, stats = GB.under_two_fills(case, only_from=(THIS,))
  assert [p for p, _ in out] == ["out['y']", "out['parts'][0]", "out['parts'][1]", "out['idx']"]
  assert torch.equal(out[0][1], 2 * torch.arange(12.0).view(3, 4)) and stats['allocations'] == [3, 3]


def test_non_finite_outputs_are_allowed_when_an_input_is_not_finite():
  def case():
    x = GB.place(torch.tensor([1.0, float('nan'), 3.0]))
    return x * 2
  GB.under_two_fills(case, only_from=(THIS,))


class _Scaled(torch.autograd.Function):

  @staticmethod
  def forward(ctx, x):
    return x * 2

  @staticmethod
  def backward(ctx, g):
    ws = torch.empty(4)
    ws.fill_(2.0)
    _Scaled.seen.append(ws)
    if _Scaled.overrun:
      _raw(ws, 16, 4).view(torch.int32)[0] = 0x12345678
    return g * ws[0]


def test_allocations_inside_a_backward_are_guarded():
  _Scaled.seen, _Scaled.overrun = [], False
  x = torch.ones(3, requires_grad=True)
  with GB.guarded(0, only_from=(THIS,)) as gb:
    _Scaled.apply(x).sum().backward()
    assert x.grad.tolist() == [2.0, 2.0, 2.0]
    assert len(gb.allocations) == 1 and gb.allocations[0].shape == (4,) and _Scaled.seen[0].data_ptr() % 256 == 0
    GB.check()
    _Scaled.overrun = True
    _Scaled.apply(x).sum().backward()
    with pytest.raises(GB.GuardError) as ei:
      GB.check()
    assert ei.value.reports[0][1:] == ('rear', 16, 19) and ei.value.reports[0][0] is gb.allocations[1]


# ------------------------------------------------------------------ the coverage ledger
def _declared_entries():
  import test_gpu_guard_bands as T  # (imports without a GPU; nothing runs)
  return set().union(*[c.entries for c in T.CASES])


def launching_entries():
  return set(mode_hip.LAUNCHING) - {'mode_debug_poison'}


def test_every_case_declares_what_it_launches():
  import test_gpu_guard_bands as T
  assert len({c.id for c in T.CASES}) == len(T.CASES)
  assert not [c.id for c in T.CASES if not c.entries]
  assert not set(T.LAUNCHES) - {c.id for c in T.CASES}, 'rows of LAUNCHES without a case'


def test_every_launching_entry_of_the_abi_has_a_guarded_case():
  declared, want = _declared_entries(), launching_entries()
  assert not declared - want, 'declared but not a launching entry of mode_hip.SIGNATURES: %s' % sorted(declared - want)
  assert not want - declared, 'no guarded case declares: %s' % sorted(want - declared)
