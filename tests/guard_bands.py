"""Guard bands: does a kernel touch memory outside the buffers it was given?  (tests/test_guard_bands_host.py, tests/test_gpu_guard_bands.py)

Inside `guarded()` the buffers that the host code allocates for the kernels -- outputs, workspaces, weight packs, tables -- come back as
contiguous views in the middle of a larger allocation, with a pattern-filled guard zone on each side.  A TorchDispatchMode sees the
factory ops (torch.empty, empty_like, empty_strided, zeros, zeros_like, ones, full, new_empty, new_zeros, clone, the copy behind
contiguous(), and the copy behind .to(device) / .to(dtype) -- that is how host-built plans and tables reach the GPU) and relocates the result of those whose nearest caller outside torch is a file of the package (mode-2022_amd/: mode_hip/,
models/, utils/).  `place(t)` puts a test's own input into the same kind of view.  `check()` compares every guard with its pattern and
names the allocation (file:line of the frame that made it, shape), the side and the first / last damaged byte.  The mode is thread
local state that the autograd engine carries to its device threads, so buffers made inside a Function.backward are guarded too.

Layout of one allocation (bytes, G = max(256 KiB, the tensor's bytes) rounded up to 256):

    [ front guard: G ][ tensor: n ][ pad to the pattern word: < 4 ][ rear guard: G ]

The front guard and the tensor start at multiples of 256 bytes (no kernel's alignment assumption changes); the rear guard begins at the
tensor's last byte rounded up to 4.  The pad bytes carry the pattern and count as rear guard.  A freshly "empty" tensor carries the
pattern too: a kernel that reads a slot nobody wrote shows like one that reads a guard.

Writes are found by `check()`.  Reads are found by `under_two_fills(fn)`: fn runs twice with different guard contents (floating-point
buffers: the quiet NaN 0x7fc00000, then 0x3f803f80; integer buffers: 1, then 2 -- small, so that an index fetched from a guard still
lands inside the allocation); the outputs must be bit-equal and finite.  A value fetched from a guard shows even under a zero weight
(NaN x 0 = NaN); one that is fetched and discarded does not, which is the right verdict for it.  A write that happens to equal one
fill's pattern is caught under the other.

What is NOT intercepted: tensors that torch's own operators produce (x + y, torch.cat, torch.stack, F.interpolate, the gradients the
autograd engine accumulates, ...) and allocations made from files outside the package.  A kernel that overruns such a tensor goes
unnoticed unless the test `place`s it.
"""
import contextlib
import os
import sys

import torch
from torch.utils._python_dispatch import TorchDispatchMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'mode-2022_amd') + os.sep
_TORCH = os.path.dirname(os.path.abspath(torch.__file__)) + os.sep
_HERE = os.path.abspath(__file__)
MIN_GUARD = 256 * 1024
ALIGN = 256
FLOAT_FILLS = (0x7fc00000, 0x3f803f80)
INT_FILLS = (1, 2)

_aten = torch.ops.aten
FACTORY_OPS = (_aten.empty.memory_format, _aten.empty_strided.default, _aten.empty_like.default, _aten.zeros.default, _aten.zeros_like.default,
               _aten.ones.default, _aten.full.default, _aten.new_empty.default, _aten.new_zeros.default, _aten.clone.default, _aten._to_copy.default)
_UNWRITTEN = (_aten.empty.memory_format, _aten.empty_strided.default, _aten.empty_like.default, _aten.new_empty.default)


def _pattern_word(dtype, fill):
  """(bytes of one pattern word, the word as a signed integer, the integer dtype to fill with)."""
  e = torch.empty((), dtype=dtype).element_size()
  if dtype.is_floating_point or dtype.is_complex:
    if e == 8 and not dtype.is_complex:
      word, n = ((0x7ff8000000000000, 0x3ff0000000000000)[fill], 8)  # float64: its own quiet NaN, then 1.0
    else:
      word, n = (FLOAT_FILLS[fill], 4)
  else:
    v = INT_FILLS[fill]
    word, n = {1: (v * 0x01010101, 4), 2: (v * 0x00010001, 4), 4: (v, 4), 8: (v, 8)}[e]
  raw = word.to_bytes(n, 'little')
  signed = int.from_bytes(raw, 'little', signed=True)
  return raw, signed, (torch.int32 if n == 4 else torch.int64)


def _dense(t):
  """Every element of the storage span belongs to t exactly once (contiguous, or a permutation of it)."""
  if t.is_contiguous():
    return True
  span = 1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride()))
  return span == t.numel() and min(t.stride()) > 0 and len(set(s for n, s in zip(t.shape, t.stride()) if n > 1)) == sum(1 for n in t.shape if n > 1)


class Guarded(object):
  """One guarded allocation: `block` is the whole byte buffer (front guard, tensor, pad, rear guard)."""

  def __init__(self, block, front, nbytes, rear_at, raw, word, wtype, where, shape, dtype, kind):
    self.block, self.front, self.nbytes, self.rear_at = block, front, nbytes, rear_at
    self.raw, self.word, self.wtype = raw, word, wtype
    self.where, self.shape, self.dtype, self.kind = where, tuple(shape), dtype, kind

  def _zones(self):
    b = self.block
    return (('front', b[:self.front].view(self.wtype), 0), ('rear', b[self.rear_at:].view(self.wtype), self.rear_at))

  def damaged_flags(self):
    flags = [(z != self.word).any() for _, z, _ in self._zones()]
    if self.rear_at > self.front + self.nbytes:
      flags.append((self._pad() != self._pad_expected()).any())
    return flags

  def _pad(self):
    return self.block[self.front + self.nbytes:self.rear_at]

  def _pad_expected(self):
    k = self.nbytes % len(self.raw)
    return torch.tensor(list(self.raw[k:]), dtype=torch.uint8, device=self.block.device)

  def damage(self):
    """[(side, first, last)]: byte offsets relative to the tensor's first byte (front: negative; rear: >= the tensor's bytes)."""
    out = []
    exp = torch.tensor(list(self.raw), dtype=torch.uint8, device=self.block.device)
    for side, zone, at in self._zones():
      zb = zone.view(torch.uint8)
      bad = (zb.view(-1, len(self.raw)) != exp).view(-1)
      if side == 'rear' and self.rear_at > self.front + self.nbytes:
        bad = torch.cat([self._pad() != self._pad_expected(), bad])
        at = self.front + self.nbytes
      idx = bad.nonzero().view(-1)
      if idx.numel():
        out.append((side, int(idx[0]) + at - self.front, int(idx[-1]) + at - self.front))
    return out

  def describe(self):
    return '%s %s %s %s (%d bytes)' % (self.kind, self.where, self.shape, str(self.dtype).replace('torch.', ''), self.nbytes)


class GuardError(AssertionError):

  def __init__(self, reports):
    self.reports = reports  # [(Guarded, side, first, last)]
    lines = ['%s: %s guard damaged, bytes %+d .. %+d relative to the tensor' % (g.describe(), side, a, b) for g, side, a, b in reports]
    AssertionError.__init__(self, '%d damaged guard(s):\n  ' % len(reports) + '\n  '.join(lines))


def _caller():
  """The nearest frame outside torch and this module: (file, line)."""
  f = sys._getframe(1)
  while f is not None:
    name = os.path.abspath(f.f_code.co_filename)
    if name != _HERE and not name.startswith(_TORCH) and not f.f_code.co_filename.startswith('<'):
      return name, f.f_lineno
    f = f.f_back
  return None, 0


class GuardBands(TorchDispatchMode):
  """The dispatch mode and the registry of what it handed out.  fill: 0 or 1 (which of the two patterns)."""

  def __init__(self, fill=0, only_from=(PKG,)):
    TorchDispatchMode.__init__(self)
    self.fill, self.only_from = fill, tuple(only_from)
    self.allocations = []
    self.placed_finite = True
    self._busy = False  # (place() and check() run with the mode active: their own allocations are not relocated)

  def __torch_dispatch__(self, func, types, args=(), kwargs=None):
    out = func(*args, **(kwargs or {}))
    if func in FACTORY_OPS and isinstance(out, torch.Tensor) and not self._busy:
      name, line = _caller()
      if name is not None and name.startswith(self.only_from):
        return self.relocate(out, '%s:%d' % (os.path.relpath(name, ROOT), line), func not in _UNWRITTEN, func.__name__.split('.')[0])
    return out

  def relocate(self, t, where, keep_content, kind):
    """A tensor of t's shape, dtype, strides and (keep_content) values in the middle of a guarded block; t itself where that cannot be done."""
    if t.numel() == 0 or t.layout != torch.strided or t.is_quantized or not _dense(t):
      return t
    nbytes = t.numel() * t.element_size()
    raw, word, wtype = _pattern_word(t.dtype, self.fill)
    unit = len(raw)
    guard = -(-max(MIN_GUARD, nbytes) // ALIGN) * ALIGN
    rear_at = guard + -(-nbytes // unit) * unit
    total = rear_at + guard
    base = torch.empty(total + ALIGN, dtype=torch.uint8, device=t.device)
    off = -base.data_ptr() % ALIGN
    block = base[off:off + total]
    block.view(wtype).fill_(word)
    view = block[guard:guard + nbytes].view(t.dtype)
    view = view.view(t.shape) if t.is_contiguous() else view.as_strided(t.shape, t.stride())
    if keep_content:
      view.copy_(t)
    self.allocations.append(Guarded(block, guard, nbytes, rear_at, raw, word, wtype, where, t.shape, t.dtype, kind))
    return view

  def place(self, t, is_input=True):
    """Copy a test's input into a guarded view (same device, dtype, shape; contiguous).  is_input=False: a buffer the operator
    writes (it may hold NaN without switching the finiteness check of under_two_fills off)."""
    name, line = _caller()
    t = t.detach()
    if is_input and t.is_floating_point() and not bool(torch.isfinite(t).all()):
      self.placed_finite = False
    self._busy = True
    try:
      with torch.no_grad():
        return self.relocate(t.contiguous(), '%s:%d' % (os.path.relpath(name, ROOT) if name else '?', line), True, 'placed')
    finally:
      self._busy = False

  def check(self):
    """Raise GuardError naming every damaged guard.  Call after torch.cuda.synchronize()."""
    self._busy = True
    try:
      flags, owner = [], []
      for g in self.allocations:
        for f in g.damaged_flags():
          flags.append(f)
          owner.append(g)
      if not flags:
        return
      hit = torch.stack(self._gather(flags))  # one transfer per device
      bad = []
      for g in dict.fromkeys(o for o, h in zip(owner, hit.tolist()) if h):
        bad += [(g,) + d for d in g.damage()]
    finally:
      self._busy = False
    if bad:
      raise GuardError(bad)

  @staticmethod
  def _gather(flags):
    by_dev = {}
    for i, f in enumerate(flags):
      by_dev.setdefault(f.device, []).append((i, f))
    out = [None] * len(flags)
    for dev, items in by_dev.items():
      got = torch.stack([f for _, f in items]).cpu()
      for (i, _), v in zip(items, got):
        out[i] = v
    return out


_active = []


@contextlib.contextmanager
def guarded(fill=0, only_from=(PKG,)):
  gb = GuardBands(fill, only_from)
  _active.append(gb)
  try:
    with gb:
      yield gb
  finally:
    _active.pop()


def current():
  assert _active, 'place() / check() need an enclosing guarded() context'
  return _active[-1]


def place(t, is_input=True):
  return current().place(t, is_input)


def check():
  return current().check()


def _leaves(x, path='out'):
  if torch.is_tensor(x):
    yield path, x
  elif isinstance(x, dict):
    for k in x:
      for item in _leaves(x[k], '%s[%r]' % (path, k)):
        yield item
  elif isinstance(x, (list, tuple)):
    for i, v in enumerate(x):
      for item in _leaves(v, '%s[%d]' % (path, i)):
        yield item
  elif isinstance(x, float):
    yield path, torch.tensor(x, dtype=torch.float64)
  elif x is not None and not isinstance(x, (int, str, bool)):
    raise TypeError('under_two_fills: %s is a %s' % (path, type(x)))


def _bits(t):
  t = t.contiguous()
  if t.is_complex():
    t = torch.view_as_real(t)
  return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def under_two_fills(fn, only_from=(PKG,)):
  """Run fn() under each of the two fills.  fn builds FRESH inputs (so that caches keyed on (data_ptr, _version) allocate inside the
  context too), `place`s them and returns tensors (nested lists / tuples / dicts; floats allowed).  Asserts: every guard intact in both
  runs; outputs bit-equal between the runs; outputs finite if every placed input was.  Returns the first run's outputs as
  [(path, CPU tensor)] and statistics {'allocations': [n0, n1]}."""
  runs, counts = [], []
  for fill in (0, 1):
    with guarded(fill, only_from) as gb:
      out = fn()
      if torch.cuda.is_available():
        torch.cuda.synchronize()
    leaves = [(p, t.detach().cpu().clone()) for p, t in _leaves(out)]  # (outside the mode: these copies are not guarded)
    gb.check()
    counts.append(len(gb.allocations))
    finite = gb.placed_finite
    del out
    if finite:
      for p, t in leaves:
        if t.is_floating_point() or t.is_complex():
          n = int((~torch.isfinite(t)).sum())
          assert n == 0, 'fill %d: %s %s has %d non-finite values although every input is finite: a guard or an unwritten buffer was read' % (
              fill, p, tuple(t.shape), n)
    runs.append(leaves)
  a, b = runs
  assert [p for p, _ in a] == [p for p, _ in b]
  for (p, x), (_, y) in zip(a, b):
    assert x.shape == y.shape and x.dtype == y.dtype, p
    if not torch.equal(_bits(x), _bits(y)):
      bad = (_bits(x) != _bits(y)).view(-1).nonzero().view(-1)
      raise AssertionError('%s %s differs between the two guard fills in %d of %d elements (first flat index %d, last %d): a guard or an '
                           'unwritten buffer was read' % (p, tuple(x.shape), bad.numel(), x.numel(), int(bad[0]), int(bad[-1])))
  return a, {'allocations': counts}
