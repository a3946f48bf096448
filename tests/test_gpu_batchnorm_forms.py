"""BatchNorm (+ add) (+ ReLU), csrc/bn_act.hip: every entry, every instantiated form and every block split against tests/bn_ref.py.

Cases.  bn_ref.GRID_CASES: the smallest (B, C, S) that reach each regime of pick_nsplit / apply_chunks (scalar rows, the 16-byte tail loop
alone, the 4 x unrolled loop with its tail, 2 and 4 blocks per row, statistics groups, the second trip of reduce_partials at 257
partials, the cap of 1024 partials with the workspace full to its last float and 1025 apply chunks).  Which regime a call ran in is read
back from the workspace: exactly the first 2 x rows x nsplit floats are written.  Every case runs relu x add in all four combinations.

Exact checks (grid inputs: every float32 partial sum is exact in any order, bn_ref's docstring).  Per (group, channel) the workspace
holds sum (y - K) and sum (y - K)^2 after the forward call, sum g and sum g y after the backward call, compared as integers -- one
16-byte piece lost or taken twice among 8.4 M elements is one unit.  save_mean / save_invstd / running statistics within 1 float32 ulp of
the float64 evaluation of the exact sums; gbeta = sum g exactly; ggamma within 1 ulp of invstd (sum g y - mean sum g) from the kernel's own
saved statistics; accumulate = 1 adds the same values to the prefill; gadd and the tracked maxima bit for bit; the workspace sits between
guard bands.  `out` against float64 y scale + shift (+ add) from the returned float32 coefficients: within 1 ulp of the result without
the add; with it the kernel rounds twice (the fma, then the add), so the bound is 1 ulp of the larger of |y scale + shift| and |result| --
1 ulp of the result alone cannot hold where the add cancels.

Float64 bounds (grid and seeded normal inputs).  Every output in max norm against bn_ref.reference: at most 4 x the error of torch's CPU
float32 batch_norm on the same inputs (bn_ref.yardstick) and never above the caps of the older tests (2e-5 / 5e-5 max / 1e-4 max).

Alignment.  The three entries refuse (B, C, S) tensors and workspaces at addresses the kernels cannot read in 16-byte pieces; the
per-channel vectors are read element by element and are not part of that contract.  models.stage3d.bn_act on a contiguous view that
starts one element into a buffer: HF copies such a tensor (mode_hip.functional._bn_rows) and the result has the aligned call's bits.

Measured on an MI355X, worst ratio (kernel error) / (yardstick) per tensor over the forms of each case: MEASURED below."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

import bn_ref as R
import guard_bands as GB
import mode_hip
from mode_hip import functional as HF

DEV = 'cuda:0'
EPS = R.EPS
SEED = 3
M01 = float(np.float32(0.1))  # the momentum the entries receive (a C float)
COMBOS = [(False, False), (True, False), (True, True), (False, True)]
GRID_IDS = ['%dx%dx%d-g%d' % (s + (g,)) for s, g, _, _ in R.GRID_CASES]
RANDOM_CASES = [(s, g) for s, g, _, _ in R.GRID_CASES if s[2] < 20000]
RANDOM_IDS = ['%dx%dx%d-g%d' % (s + (g,)) for s, g in RANDOM_CASES]

# Worst (kernel error) / (yardstick) over the forms of each case, MI355X.  gadd is exact everywhere (0 / 0), gbeta on the grid too.
MEASURED = """
inputs          (B, C, S) groups      out    gy     ggamma  gbeta
grid            (2, 3, 7) 1           0.51   1.59   1.00    0
grid            (1, 2, 1031) 1        1.00   1.12   0.85    0
grid            (2, 4, 3072) 1        1.00   0.89   0.23    0
grid            (2, 3, 4100) 1        1.00   0.91   0.08    0
grid            (1, 3, 16392) 1       0.87   0.85   0.15    0
grid            (4, 2, 16392) 2       0.78   1.01   0.08    0
grid            (6, 2, 16392) 3       0.89   0.99   0.35    0
grid            (1, 2, 32769) 1       1.00   1.04   0.07    0
grid            (1, 2, 2105348) 1     0.87   0.50   0.01    0
grid            (1, 1, 8396804) 1     1.00   0.89   0.00    0
grid, eval      all ten               1.00
normal          (2, 3, 7) 1           1.49   2.00   2.66    1.00
normal          (1, 2, 1031) 1        1.33   0.96   1.88    0.50
normal          (2, 4, 3072) 1        1.91   1.45   0.81    0.76
normal          (2, 3, 4100) 1        1.32   1.22   0.43    0.69
normal          (1, 3, 16392) 1       1.14   1.49   0.75    0.18
normal          (4, 2, 16392) 2       0.91   1.36   0.52    0.14
normal          (6, 2, 16392) 3       1.17   1.36   0.29    0.16
mean-dominated  (4, 2, 4100) 2        0.51   1.41   1.01    0.55
mean-dominated  (2, 2, 16392) 2       0.60   2.22   1.00    0.16
HF.bn_act on the first five cases: the figures of `normal`.
Yardsticks are of the order 1e-7 .. 6e-7 for out and gy, 1e-6 .. 4e-4 for the affine gradients (their sums grow with the count), and
1e-4 / 1e-5 / 1e-2 for out / gy / ggamma of the mean-dominated channels.

The mean-dominated cases are what changed the kernels: with sum g y taken unshifted in float32 (the backward reduce pass as it was) they
measured gy 4.3 / 11.1 / 7.9 / 10.4 and ggamma 1.9 / 7.1 / 8.1 / 14.0 times the yardstick (ggamma of the mean -3000 channel 4e-3 off,
relative) -- beyond 4 x.  Where |mean| > 16 std the pass now sums g (y - K) around the forward's pivot and the apply pass adds
(mean - K) sum g back in double; every other channel keeps the unshifted sum and with it the bits it always had.
"""


@pytest.fixture
def _stop_at_a_gpu_fault():
  """As tests/test_gpu_guard_bands.py (not autouse here: this file has a CPU-tier test): if the device no longer answers after a test,
  the session ends there."""
  yield
  try:
    torch.cuda.synchronize()
  except RuntimeError as e:
    pytest.exit('the GPU reported an error after this test; nothing more is started on it: %s' % e, returncode=3)


def gpu(fn):
  return pytest.mark.gpu(pytest.mark.usefixtures('_stop_at_a_gpu_fault')(fn))


def _ptr(t):
  return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _nan(*shape):
  return torch.full(shape, float('nan'), device=DEV)


def _ws_floats(rows):
  return mode_hip.lib().mode_bn_workspace_bytes(rows) // 4


def _dev(c):
  return {k: c[k].to(DEV) for k in ('y', 'add', 'gout', 'gamma', 'beta')}


def _forward(d, shape, groups, relu, with_add, ws, amax=False, coef=True, running=None, momentum=M01, y=None):
  """One call of mode_bn_train_fwd[_amax] into NaN-prefilled outputs.  running: (running_mean, running_var, num_batches_tracked)."""
  lib = mode_hip.lib()
  B, C, S = shape
  y = d['y'] if y is None else y
  r = {'out': torch.full_like(y, float('nan')), 'mean': _nan(groups * C), 'invstd': _nan(groups * C), 'scale': _nan(groups * C) if coef else None,
       'shift': _nan(groups * C) if coef else None, 'amax': _nan(HF.BN_ABSMAX_FLOATS) if amax else None}
  rm, rv, nbt = running if running is not None else (None, None, None)
  args = (_ptr(y), _ptr(d['add']) if with_add else None, _ptr(d['gamma']), _ptr(d['beta']), _ptr(rm), _ptr(rv), _ptr(nbt), momentum, EPS, int(relu),
          _ptr(r['out']), _ptr(r['mean']), _ptr(r['invstd']), _ptr(r['scale']), _ptr(r['shift']), _ptr(ws), B, C, S, groups)
  rc = lib.mode_bn_train_fwd_amax(*args, _ptr(r['amax']), None) if amax else lib.mode_bn_train_fwd(*args, None)
  assert rc == 0, lib.mode_last_error()
  torch.cuda.synchronize()
  return r


def _backward(d, f, shape, groups, mode, with_gadd, ws, accumulate=None, amax=True, gout=None):
  """One call of mode_bn_train_bwd[_amax] behind the forward f.  mode 0: no ReLU; 1: mask from f['out']; 2: mask from y and f's
  coefficients.  accumulate: None, or the (ggamma, gbeta) prefill to add into."""
  lib = mode_hip.lib()
  B, C, S = shape
  gout = d['gout'] if gout is None else gout
  r = {'gy': torch.full_like(d['y'], float('nan')), 'gadd': torch.full_like(d['y'], float('nan')) if with_gadd else None,
       'ggamma': accumulate[0].clone() if accumulate else _nan(C), 'gbeta': accumulate[1].clone() if accumulate else _nan(C),
       'amax': _nan(HF.BN_ABSMAX_FLOATS) if amax else None}
  out = f['out'] if mode == 1 else None
  sc, sh = (f['scale'], f['shift']) if mode == 2 else (None, None)
  args = (_ptr(gout), _ptr(d['y']), _ptr(out), _ptr(d['gamma']), _ptr(f['mean']), _ptr(f['invstd']), _ptr(sc), _ptr(sh), int(mode != 0), _ptr(r['gy']),
          _ptr(r['gadd']), _ptr(r['ggamma']), _ptr(r['gbeta']), 1 if accumulate else 0, _ptr(ws), B, C, S, groups)
  rc = lib.mode_bn_train_bwd_amax(*args, _ptr(r['amax']), None) if amax else lib.mode_bn_train_bwd(*args, None)
  assert rc == 0, lib.mode_last_error()
  torch.cuda.synchronize()
  return r


def _row_sums(ws, rows, nsplit, unit0, unit1):
  """The workspace as integers: per row the totals of its even and of its odd floats in units of unit0 / unit1, and the set of pairs
  that hold anything.  Every float must be a whole number of units."""
  w = ws.cpu().double().numpy().reshape(-1, 2)
  a, b = w[:, 0] / unit0, w[:, 1] / unit1
  assert np.array_equal(a, np.rint(a)) and np.array_equal(b, np.rint(b)), 'a partial sum is no whole multiple of the grid unit'
  used = rows * nsplit
  assert not w[used:].any(), 'the workspace is written behind the %d x %d partial pairs of this launch geometry' % (rows, nsplit)
  return a[:used].reshape(rows, nsplit).sum(1).astype(np.int64), b[:used].reshape(rows, nsplit).sum(1).astype(np.int64), b[:used] != 0


def _err(got, ref_dev):
  return float((got.double() - ref_dev).abs().max())


def _report(tag, errs, yard, refs, caps=R.CAPS):
  """Print error / yardstick per tensor, then hold each to min(4 x yardstick, the older tests' cap)."""
  line = '  '.join('%s %.2e/%.2e' % (k, errs[k], yard[k]) for k in errs)
  print('%s: kernel error / yardstick: %s' % (tag, line))
  for k in errs:
    b = R.bound(k, yard, refs[k], caps)
    assert errs[k] <= b, '%s: %s is %.3e off float64, bound %.3e (yardstick %.3e)' % (tag, k, errs[k], b, yard[k])


def _check_out(f, d, relu, with_add, y=None):
  """out against float64 y scale + shift (+ add) from the returned coefficients (module docstring); nothing left NaN."""
  y = d['y'] if y is None else y
  B, C, S = y.shape
  G = f['scale'].numel() // C
  sc = f['scale'].double().view(G, 1, C, 1).expand(G, B // G, C, 1).reshape(B, C, 1)
  sh = f['shift'].double().view(G, 1, C, 1).expand(G, B // G, C, 1).reshape(B, C, 1)
  t = y.double() * sc + sh
  want = t + d['add'].double() if with_add else t
  want = torch.relu(want) if relu else want
  assert not bool(torch.isnan(f['out']).any())
  scale_of = torch.maximum(t.abs(), want.abs()) if with_add else want.abs()
  ulp = torch.from_numpy(R.ulp32(scale_of.cpu().numpy())).to(DEV)
  worst = float(((f['out'].double() - want).abs() / ulp).max())
  assert worst <= 1.0, 'out is %.2f ulp off y * scale + shift' % worst


def _modes(relu, with_add):
  if not relu:
    return [(0, False), (0, True)]
  return [(1, False), (1, True)] if with_add else [(1, False), (1, True), (2, False), (2, True)]


# ------------------------------------------------------------------------------------------------ every form on the grid cases
@gpu
@pytest.mark.parametrize('relu,with_add', COMBOS)
@pytest.mark.parametrize('shape,groups,step,span', R.GRID_CASES, ids=GRID_IDS)
def test_grid_every_form(shape, groups, step, span, relu, with_add):
  B, C, S = shape
  rows = C * groups
  c = R.grid_case(shape, groups, SEED, step, span)
  ref = R.reference(c, relu, with_add, groups)
  yard = R.yardstick(c, relu, with_add, groups, ref)
  nsplit, chunks = R.GRID_GEOMETRY[(shape, groups)]
  d = _dev(c)
  tag = 'grid %s g%d relu%d add%d' % (shape, groups, relu, with_add)
  mean_x, var_x, count = R.exact_statistics(c)
  s0, s1 = R.exact_forward_sums(c)
  exact = {'mean': torch.from_numpy(mean_x), 'var': torch.from_numpy(var_x), 'count': count}
  rm0, rv0 = torch.arange(1, C + 1, dtype=torch.float32) * 0.25, torch.arange(1, C + 1, dtype=torch.float32) * 0.5 + 0.25

  # ---- forward: statistics, workspace, running statistics, out
  with GB.guarded() as gb:
    ws = GB.place(torch.zeros(_ws_floats(rows), device=DEV))
    running = (rm0.to(DEV), rv0.to(DEV), torch.tensor(5, dtype=torch.int64, device=DEV))
    f = _forward(d, shape, groups, relu, with_add, ws, running=running)
    gb.check()
  t0, t1, written = _row_sums(ws, rows, nsplit, step, step * step)
  assert written.all(), 'a statistics block of the %d per row left its slot unwritten' % nsplit
  assert np.array_equal(t0, s0.reshape(-1)) and np.array_equal(t1, s1.reshape(-1)), 'the statistics pass lost or repeated elements'
  invstd_x = 1.0 / np.sqrt(var_x + EPS)
  assert (np.abs(f['mean'].cpu().double().numpy() - mean_x.reshape(-1)) <= R.ulp32(mean_x.reshape(-1))).all()
  assert (np.abs(f['invstd'].cpu().double().numpy() - invstd_x.reshape(-1)) <= R.ulp32(invstd_x.reshape(-1))).all()
  rm_x, rv_x = R.running_update(exact, rm0, rv0, M01)
  assert (np.abs(running[0].cpu().double().numpy() - rm_x.double().numpy()) <= R.ulp32(rm_x)).all()
  assert (np.abs(running[1].cpu().double().numpy() - rv_x.double().numpy()) <= R.ulp32(rv_x)).all()
  assert int(running[2]) == 5 + groups
  _check_out(f, d, relu, with_add)
  refs = {k: ref[k].to(DEV) for k in ('out', 'gy', 'gadd', 'ggamma', 'gbeta')}
  _report(tag + ' fwd', {'out': _err(f['out'], refs['out'])}, yard, refs)

  # ---- the other forms of the forward: momentum 1, the tracked maximum, no saved coefficients -- the same bits
  ws2 = torch.zeros(_ws_floats(rows), device=DEV)
  running1 = (rm0.to(DEV), rv0.to(DEV), None)
  for amax, coef, run, mom in ((True, True, running1, 1.0), (True, False, None, M01), (False, False, None, M01)):
    v = _forward(d, shape, groups, relu, with_add, ws2, amax=amax, coef=coef, running=run, momentum=mom)
    for k in ('out', 'mean', 'invstd') + (('scale', 'shift') if coef else ()):
      assert torch.equal(v[k], f[k]), '%s differs between the forms of the forward (amax %d, coefficients %d)' % (k, amax, coef)
    if amax:
      assert float(v['amax'].max()) == float(v['out'].abs().max())
  rm_1, rv_1 = R.running_update(exact, rm0, rv0, 1.0)
  assert (np.abs(running1[0].cpu().double().numpy() - rm_1.double().numpy()) <= R.ulp32(rm_1)).all()
  assert (np.abs(running1[1].cpu().double().numpy() - rv_1.double().numpy()) <= R.ulp32(rv_1)).all()

  # ---- eval mode on the running statistics just written
  lib = mode_hip.lib()
  e = torch.full_like(d['y'], float('nan'))
  rc = lib.mode_bn_eval_fwd(_ptr(d['y']), _ptr(d['add']) if with_add else None, _ptr(d['gamma']), _ptr(d['beta']), _ptr(running[0]), _ptr(running[1]), EPS,
                            int(relu), _ptr(e), B, C, S, None)
  assert rc == 0, lib.mode_last_error()
  torch.cuda.synchronize()
  e_ref = R.eval_forward(c['y'], c['gamma'], c['beta'], running[0].cpu(), running[1].cpu(), c['add'] if with_add else None, relu)
  e_yard = R.eval_yardstick(c['y'], c['gamma'], c['beta'], running[0].cpu(), running[1].cpu(), c['add'] if with_add else None, relu, e_ref)
  _report(tag + ' eval', {'out': _err(e, e_ref.to(DEV))}, {'out': e_yard}, {'out': e_ref})
  del e, e_ref

  # ---- backward: every mask source, with and without the skip gradient, stored and accumulated
  mask = (ref['pre'] > 0).numpy() if relu else None
  g0, g1 = R.exact_backward_sums(c, mask)
  assert np.abs(g0.sum(0)).max() < 2**24
  gbeta_x = torch.from_numpy((g0.sum(0) * step).astype(np.float32)).to(DEV)
  masked = torch.where(f['out'] > 0, d['gout'], torch.zeros_like(d['gout'])) if relu else d['gout']
  worst = {}
  for mode, with_gadd in _modes(relu, with_add):
    with GB.guarded() as gb:
      ws = GB.place(torch.zeros(_ws_floats(rows), device=DEV))
      b = _backward(d, f, shape, groups, mode, with_gadd, ws)
      gb.check()
    t0, t1, _ = _row_sums(ws, rows, nsplit, step, step * step)
    # (the pass sums g (y - K), K the forward's pivot where |mean| > 16 std and 0 elsewhere -- the grid's channels: sum g y is that + K sum g)
    shifted = (f['mean'].abs() * f['invstd'] > 16).cpu().numpy()
    t1 = t1 + np.where(shifted, c['K'].reshape(-1), 0) * t0
    assert np.array_equal(t0, g0.reshape(-1)) and np.array_equal(t1, g1.reshape(-1)), 'mode %d: the reduce pass lost or repeated elements' % mode
    assert torch.equal(b['gbeta'], gbeta_x), 'mode %d: gbeta is not the exact sum of the masked gradient' % mode
    m64, i64 = f['mean'].double().cpu().numpy().reshape(groups, C), f['invstd'].double().cpu().numpy().reshape(groups, C)
    gg = (i64 * (g1 * step * step - m64 * (g0 * step))).sum(0)
    assert (np.abs(b['ggamma'].cpu().double().numpy() - gg) <= R.ulp32(gg)).all(), 'mode %d: ggamma' % mode
    assert not bool(torch.isnan(b['gy']).any())
    assert float(b['amax'].max()) == float(b['gy'].abs().max())
    if with_gadd:
      assert torch.equal(b['gadd'], masked), 'mode %d: gadd is not the masked gradient bit for bit' % mode
    pre_g, pre_b = torch.arange(C, dtype=torch.float32, device=DEV) * 0.75 - 1.0, torch.arange(C, dtype=torch.float32, device=DEV) * -1.5 + 2.0
    a = _backward(d, f, shape, groups, mode, with_gadd, ws2, accumulate=(pre_g, pre_b), amax=False)  # (the plain entry)
    assert torch.equal(a['ggamma'], pre_g + b['ggamma']) and torch.equal(a['gbeta'], pre_b + b['gbeta']), 'mode %d: accumulate' % mode
    assert torch.equal(a['gy'], b['gy']) and (not with_gadd or torch.equal(a['gadd'], b['gadd']))
    errs = {k: _err(b[k], refs[k]) for k in ('gy', 'ggamma', 'gbeta')}
    if with_gadd and with_add:
      errs['gadd'] = _err(b['gadd'], refs['gadd'])
    _report('%s bwd mode %d gadd %d' % (tag, mode, with_gadd), errs, yard, refs)
    for k in errs:
      worst[k] = max(worst.get(k, 0.0), errs[k])
  print('%s worst: %s' % (tag, '  '.join('%s %.2f' % (k, worst[k] / yard[k] if yard[k] else 0.0) for k in worst)))


# ------------------------------------------------------------------------------------------------ seeded normal inputs
@gpu
@pytest.mark.parametrize('relu,with_add', COMBOS)
@pytest.mark.parametrize('shape,groups', RANDOM_CASES, ids=RANDOM_IDS)
def test_random_every_form_against_float64(shape, groups, relu, with_add):
  _float64_forms(R.random_case(shape, groups), shape, groups, relu, with_add, 'normal %s g%d relu%d add%d' % (shape, groups, relu, with_add))


def _float64_forms(c, shape, groups, relu, with_add, tag, caps=R.CAPS):
  B, C, S = shape
  ref = R.reference(c, relu, with_add, groups)
  yard = R.yardstick(c, relu, with_add, groups, ref)
  refs = {k: ref[k].to(DEV) for k in ('out', 'gy', 'gadd', 'ggamma', 'gbeta')}
  d = _dev(c)
  ws = torch.zeros(_ws_floats(C * groups), device=DEV)
  f = _forward(d, shape, groups, relu, with_add, ws, amax=True)
  assert float(f['amax'].max()) == float(f['out'].abs().max())
  _check_out(f, d, relu, with_add)
  _report(tag + ' fwd', {'out': _err(f['out'], refs['out'])}, yard, refs, caps)
  for mode, with_gadd in _modes(relu, with_add):
    b = _backward(d, f, shape, groups, mode, with_gadd, ws)
    assert float(b['amax'].max()) == float(b['gy'].abs().max())
    errs = {k: _err(b[k], refs[k]) for k in ('gy', 'ggamma', 'gbeta')}
    if with_gadd and with_add:
      errs['gadd'] = _err(b['gadd'], refs['gadd'])
    _report('%s bwd mode %d gadd %d' % (tag, mode, with_gadd), errs, yard, refs, caps)


MEAN_DOMINATED = dict(mean=(100.0, -3000.0), std=(0.1, 0.5), margin=2e-3, clear=True)  # (2e-3: what `out` may be off, bn_ref.MEAN_DOMINATED_CAPS)


@gpu
@pytest.mark.parametrize('relu,with_add', [(True, True), (True, False)])  # (the mask from `out` behind the add: mode 1; from y: modes 1 and 2)
@pytest.mark.parametrize('shape', [(4, 2, 4100), (2, 2, 16392)])
def test_mean_dominated_channels(shape, relu, with_add):
  """mean 100 / std 0.1 and mean -3000 / std 0.5, two statistics groups, ReLU: the backward pass sums g y unshifted in float32 -- out, gy
  and the affine gradients against float64 under the same rule."""
  c = R.random_case(shape, 2, seed=81, **MEAN_DOMINATED)
  _float64_forms(c, shape, 2, relu, with_add, 'mean-dominated %s relu%d add%d' % (shape, relu, with_add), R.MEAN_DOMINATED_CAPS)


# ------------------------------------------------------------------------------------------------ NaN / Inf
@gpu
@pytest.mark.parametrize('plant', [float('nan'), float('inf')])
@pytest.mark.parametrize('shape,groups,step,span', [p for p in R.GRID_CASES if p[0][1] > 1], ids=[i for i, p in zip(GRID_IDS, R.GRID_CASES) if p[0][1] > 1])
def test_a_plant_in_one_channel_leaves_the_others_alone(shape, groups, step, span, plant):
  """A NaN or an Inf in channel 0 (one element of the last sample): every other channel of every output has the bits of the run
  without it."""
  B, C, S = shape
  c = R.grid_case(shape, groups, SEED, step, span)
  d = _dev(c)
  ws = torch.zeros(_ws_floats(C * groups), device=DEV)
  runs = []
  for planted in (False, True):
    y = d['y'].clone()
    if planted:
      y[B - 1, 0, S // 2] = plant
    dd = dict(d, y=y)
    f = _forward(dd, shape, groups, True, True, ws)
    b = _backward(dd, f, shape, groups, 1, True, ws)
    runs.append((f, b))
  (f0, b0), (f1, b1) = runs
  bits = lambda t: t.view(torch.int32)
  for k in ('out',):
    assert torch.equal(bits(f0[k][:, 1:]), bits(f1[k][:, 1:])), k
  for k in ('mean', 'invstd', 'scale', 'shift'):
    assert torch.equal(bits(f0[k].view(groups, C)[:, 1:]), bits(f1[k].view(groups, C)[:, 1:])), k
  for k in ('gy', 'gadd'):
    assert torch.equal(bits(b0[k][:, 1:]), bits(b1[k][:, 1:])), k
  for k in ('ggamma', 'gbeta'):
    assert torch.equal(bits(b0[k][1:]), bits(b1[k][1:])), k
  assert not bool(torch.isfinite(f1['out'][B - 1, 0]).all())  # (the plant did reach its own channel)


@gpu
def test_the_tracked_maximum_of_an_all_nan_tensor_is_zero():
  shape = (2, 3, 4100)
  B, C, S = shape
  c = R.grid_case(shape, 1, SEED, 0.125, 1.0)
  d = _dev(c)
  d['y'] = torch.full_like(d['y'], float('nan'))
  ws = torch.zeros(_ws_floats(C), device=DEV)
  f = _forward(d, shape, 1, False, False, ws, amax=True)
  assert bool(torch.isnan(f['out']).all()) and float(f['amax'].max()) == 0.0 and not bool(torch.isnan(f['amax']).any())
  b = _backward(d, f, shape, 1, 0, False, ws)
  assert bool(torch.isnan(b['gy']).all()) and float(b['amax'].max()) == 0.0 and not bool(torch.isnan(b['amax']).any())


# ------------------------------------------------------------------------------------------------ the two mask sources at the threshold
@gpu
@pytest.mark.parametrize('shape', [(2, 3, 4100), (1, 3, 16392)])
def test_mask_from_y_is_the_mask_from_out_at_the_threshold(shape):
  """64 elements per channel are the float32 neighbours (+-1, +-2 ulps) of the ReLU threshold -shift / scale.  Planting them moves the
  statistics and with them the threshold, so the forward is rerun and the plants renewed until they sit on it.  There the mask rebuilt
  from y and the saved coefficients (mode 2) must be the mask read from `out` (mode 1).  (Not compared with float64.)"""
  B, C, S = shape
  c = R.grid_case(shape, 1, SEED, 0.125, 1.0)
  d = _dev(c)
  y = d['y'].clone()
  ws = torch.zeros(_ws_floats(C), device=DEV)
  rs = np.random.RandomState(5)
  where = torch.from_numpy(np.stack([rs.choice(B * S - 1, 64, replace=False) + 1 for _ in range(C)])).to(DEV)  # (C, 64) flat (b, s), not the pivot
  steps = torch.tensor([1, -1, 2, -2] * 16, device=DEV)
  for _ in range(12):
    f = _forward(d, shape, 1, True, False, ws, y=y)
    t = (-f['shift'].double() / f['scale'].double()).float()  # (C,)
    plants = t[:, None].expand(C, 64).contiguous()
    for k in (1, 2):
      up, down = torch.nextafter(plants, torch.full_like(plants, float('inf'))), torch.nextafter(plants, torch.full_like(plants, float('-inf')))
      plants = torch.where(steps[None, :] >= k, up, torch.where(steps[None, :] <= -k, down, plants))
    old = y.clone()
    for ch in range(C):
      y[where[ch] // S, ch, where[ch] % S] = plants[ch]
    if torch.equal(old, y):
      break
  f = _forward(d, shape, 1, True, False, ws, y=y)
  pre = _forward(d, shape, 1, False, False, ws, y=y)['out']
  for ch in range(C):
    near = pre[:, ch][pre[:, ch].abs() < 1e-6]
    assert near.numel() >= 16 and bool((near > 0).any()) and bool((near < 0).any()), 'channel %d: %d elements on the threshold' % (ch, near.numel())
  dd = dict(d, y=y)
  one = _backward(dd, f, shape, 1, 1, False, ws)
  two = _backward(dd, f, shape, 1, 2, False, ws)
  two_gadd = _backward(dd, f, shape, 1, 2, True, ws)
  assert torch.equal(one['gbeta'], two['gbeta']) and torch.equal(one['gbeta'], two_gadd['gbeta'])
  assert torch.equal(two_gadd['gadd'], torch.where(f['out'] > 0, d['gout'], torch.zeros_like(d['gout'])))


# ------------------------------------------------------------------------------------------------ precomputed statistics
@gpu
@pytest.mark.parametrize('relu,with_add', COMBOS)
@pytest.mark.parametrize('nsplit', [1, 300, 1023])
def test_precomputed_statistics(nsplit, relu, with_add):
  """mode_bn_train_fwd_prestats[_amax] on partial sums and pivots the test writes: `nsplit` pairs per channel, then the C pivots behind
  all the pairs.  The pivot is NOT the channel's first element (three steps beside it)."""
  shape, step = (2, 3, 4100), 0.125
  B, C, S = shape
  c = R.grid_case(shape, 1, SEED, step, 1.0)
  d = _dev(c)
  piv = np.where(c['K'][0] <= 0, c['K'][0] + 3, c['K'][0] - 3)
  assert (piv != c['K'][0]).all() and (piv != c['yi'][0, :, 0]).all()
  rel = (c['yi'] - piv[None, :, None]).transpose(1, 0, 2).reshape(C, B * S)
  ws_host = np.full(_ws_floats(C), np.nan, dtype=np.float32)
  for ch in range(C):
    for i, part in enumerate(np.array_split(rel[ch], nsplit)):
      ws_host[(ch * nsplit + i) * 2] = part.sum() * step
      ws_host[(ch * nsplit + i) * 2 + 1] = (part * part).sum() * step * step
      assert (part * part).sum() < 2**24
  ws_host[2 * C * nsplit:2 * C * nsplit + C] = piv * step
  mean_x, var_x, count = R.exact_statistics(c)
  exact = {'mean': torch.from_numpy(mean_x), 'var': torch.from_numpy(var_x), 'count': count}
  invstd_x = 1.0 / np.sqrt(var_x + EPS)
  lib = mode_hip.lib()
  outs = []
  for amax in (False, True):
    with GB.guarded() as gb:
      ws = GB.place(torch.from_numpy(ws_host).to(DEV))
      rm, rv, nbt = torch.zeros(C, device=DEV), torch.ones(C, device=DEV), torch.tensor(0, dtype=torch.int64, device=DEV)
      r = {'out': torch.full_like(d['y'], float('nan')), 'mean': _nan(C), 'invstd': _nan(C), 'scale': _nan(C), 'shift': _nan(C), 'amax': _nan(HF.BN_ABSMAX_FLOATS)}
      args = (_ptr(d['y']), _ptr(d['add']) if with_add else None, _ptr(d['gamma']), _ptr(d['beta']), _ptr(rm), _ptr(rv), _ptr(nbt), M01, EPS, int(relu),
              _ptr(r['out']), _ptr(r['mean']), _ptr(r['invstd']), _ptr(r['scale']), _ptr(r['shift']), _ptr(ws), nsplit, B, C, S)
      rc = lib.mode_bn_train_fwd_prestats_amax(*args, _ptr(r['amax']), None) if amax else lib.mode_bn_train_fwd_prestats(*args, None)
      assert rc == 0, lib.mode_last_error()
      torch.cuda.synchronize()
      gb.check()
    assert torch.equal(ws.view(torch.int32), torch.from_numpy(ws_host).to(DEV).view(torch.int32)), 'the entry wrote into the statistics it was given'
    assert (np.abs(r['mean'].cpu().double().numpy() - mean_x[0]) <= R.ulp32(mean_x[0])).all()
    assert (np.abs(r['invstd'].cpu().double().numpy() - invstd_x[0]) <= R.ulp32(invstd_x[0])).all()
    rm_x, rv_x = R.running_update(exact, torch.zeros(C), torch.ones(C), M01)
    assert (np.abs(rm.cpu().double().numpy() - rm_x.double().numpy()) <= R.ulp32(rm_x)).all()
    assert (np.abs(rv.cpu().double().numpy() - rv_x.double().numpy()) <= R.ulp32(rv_x)).all()
    assert int(nbt) == 1
    _check_out(r, d, relu, with_add)
    if amax:
      assert float(r['amax'].max()) == float(r['out'].abs().max())
    outs.append(r)
  for k in ('out', 'mean', 'invstd', 'scale', 'shift'):
    assert torch.equal(outs[0][k], outs[1][k]), k


def test_precomputed_statistics_refuse_a_count_without_room_for_the_pivots():
  """0 and 1024 pairs per channel (1024 would put the pivots behind the workspace): refused before any pointer is looked at."""
  lib = mode_hip.lib()
  p = ctypes.c_void_p(0x10000)
  for entry, tail in ((lib.mode_bn_train_fwd_prestats, (None,)), (lib.mode_bn_train_fwd_prestats_amax, (p, None))):
    for nsplit in (0, 1024, -1):
      rc = entry(p, None, p, p, None, None, None, 0.1, EPS, 0, ctypes.c_void_p(0x20000), p, p, None, None, ctypes.c_void_p(0x30000), nsplit, 2, 3, 64, *tail)
      assert rc == -1 and b'partial pairs per channel' in lib.mode_last_error(), nsplit


# ------------------------------------------------------------------------------------------------ module semantics through HF.bn_act
def _pair(C, dims=4, **kw):
  BN = nn.BatchNorm3d if dims == 5 else nn.BatchNorm2d
  ref, dev = BN(C, **kw).double(), BN(C, **kw).to(DEV)
  g = torch.Generator().manual_seed(7)
  gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
  with torch.no_grad():
    for bn in (ref, dev):
      bn.weight.copy_(gamma)
      bn.bias.copy_(beta)
  return ref, dev


def _same_state(ref, dev):
  if ref.running_mean is None:
    assert dev.running_mean is None and dev.running_var is None
    return
  assert float((dev.running_mean.cpu().double() - ref.running_mean).abs().max()) < 1e-5
  assert float((dev.running_var.cpu().double() - ref.running_var).abs().max()) < 1e-4
  assert int(dev.num_batches_tracked) == int(ref.num_batches_tracked)


@gpu
@pytest.mark.parametrize('host_counter', [False, True])
@pytest.mark.parametrize('momentum', [None, 0.1])
def test_module_state_over_three_calls(momentum, host_counter):
  """momentum=None (the cumulative average needs the count on the host) and a num_batches_tracked that lives on the CPU."""
  shape = (2, 3, 4, 5, 41)
  ref, dev = _pair(3, 5, momentum=momentum)
  if host_counter:
    dev.num_batches_tracked = dev.num_batches_tracked.cpu()
  for call in range(3):
    y = R._rand(shape, 60 + call, 2.0) + 1.5
    with torch.no_grad():
      want = torch.relu(ref(y.double()))
      got = HF.bn_act(dev, y.to(DEV), None, True)
    assert float((got.cpu().double() - want).abs().max()) < 2e-5
    _same_state(ref, dev)
  assert int(dev.num_batches_tracked) == 3 and dev.num_batches_tracked.is_cuda != host_counter


@gpu
@pytest.mark.parametrize('training', [True, False])
def test_module_without_tracked_statistics(training):
  shape = (2, 3, 33, 31)
  ref, dev = _pair(3, 4, track_running_stats=False)
  ref.train(training)
  dev.train(training)
  y, add = R._rand(shape, 64, 2.0) + 1.5, R._rand(shape, 65)
  with torch.no_grad():
    want = torch.relu(ref(y.double()) + add.double())
    got = HF.bn_act(dev, y.to(DEV), add.to(DEV), True)
  assert float((got.cpu().double() - want).abs().max()) < 2e-5
  _same_state(ref, dev)


@gpu
def test_module_eval_with_add_and_relu_and_grouped_cumulative_average():
  shape = (4, 3, 33, 31)
  ref, dev = _pair(3, 4)
  y, add = R._rand(shape, 66, 2.0) + 1.5, R._rand(shape, 67)
  with torch.no_grad():
    ref(y.double())
    HF.bn_act(dev, y.to(DEV))
    ref.eval()
    dev.eval()
    want = torch.relu(ref(y.double()) + add.double())
    got = HF.bn_act(dev, y.to(DEV), add.to(DEV), True)
  assert float((got.cpu().double() - want).abs().max()) < 2e-5
  _same_state(ref, dev)
  _, cma = _pair(3, 4, momentum=None)
  with pytest.raises(NotImplementedError):
    HF.bn_act(cma, y.to(DEV), None, False, groups=2)
  assert int(cma.num_batches_tracked) == 0


@gpu
@pytest.mark.parametrize('relu,with_add', COMBOS)
@pytest.mark.parametrize('shape,groups,step,span', R.GRID_CASES[:5], ids=GRID_IDS[:5])
def test_bn_act_end_to_end(shape, groups, step, span, relu, with_add):
  """HF.bn_act (forward, autograd backward, module state) on the first five cases, seeded normal inputs, against float64."""
  B, C, S = shape
  c = R.random_case(shape, groups)
  ref = R.reference(c, relu, with_add, groups)
  yard = R.yardstick(c, relu, with_add, groups, ref)
  dev = nn.BatchNorm2d(C).to(DEV)
  with torch.no_grad():
    dev.weight.copy_(c['gamma'])
    dev.bias.copy_(c['beta'])
  y = c['y'].to(DEV).view(B, C, S, 1).requires_grad_(True)
  add = c['add'].to(DEV).view(B, C, S, 1).requires_grad_(True) if with_add else None
  out = HF.bn_act(dev, y, add, relu, groups=groups)
  out.backward(c['gout'].to(DEV).view(B, C, S, 1))
  refs = {k: ref[k].to(DEV) for k in ('out', 'gy', 'gadd', 'ggamma', 'gbeta')}
  errs = {'out': _err(out.detach().view(B, C, S), refs['out']), 'gy': _err(y.grad.view(B, C, S), refs['gy']),
          'ggamma': _err(dev.weight.grad, refs['ggamma']), 'gbeta': _err(dev.bias.grad, refs['gbeta'])}
  if with_add:
    errs['gadd'] = _err(add.grad.view(B, C, S), refs['gadd'])
  _report('bn_act %s relu%d add%d' % (shape, relu, with_add), errs, yard, refs)
  rm_x, rv_x = R.running_update(ref, torch.zeros(C), torch.ones(C), 0.1)
  assert float((dev.running_mean.cpu() - rm_x).abs().max()) < 1e-5 and float((dev.running_var.cpu() - rv_x).abs().max()) < 1e-4
  assert int(dev.num_batches_tracked) == groups


# ------------------------------------------------------------------------------------------------ refusals (made-up addresses: nothing runs)
A = {k: 0x100000 * (i + 1) for i, k in enumerate(('y', 'add', 'out', 'gout', 'gy', 'gadd', 'ws', 'vec', 'vec2'))}


def _fwd_call(lib, S, B=2, C=4, groups=1, amax=False, **over):
  a = dict(A, **over)
  p = lambda k: ctypes.c_void_p(a[k]) if a[k] is not None else None
  a.setdefault('rm', A['vec'])
  a.setdefault('rv', A['vec'])
  a.setdefault('scale', A['vec'])
  a.setdefault('shift', A['vec'])
  args = (p('y'), p('add'), p('vec'), p('vec'), p('rm'), p('rv'), None, 0.1, EPS, 1, p('out'), p('vec'), p('vec'), p('scale'), p('shift'), p('ws'), B, C, S, groups)
  return lib.mode_bn_train_fwd_amax(*args, p('vec2'), None) if amax else lib.mode_bn_train_fwd(*args, None)


def _eval_call(lib, S, B=2, C=4, **over):
  a = dict(A, **over)
  p = lambda k: ctypes.c_void_p(a[k]) if a[k] is not None else None
  return lib.mode_bn_eval_fwd(p('y'), p('add'), p('vec'), p('vec'), p('vec'), p('vec'), EPS, 1, p('out'), B, C, S, None)


def _bwd_call(lib, S, B=2, C=4, groups=1, amax=False, **over):
  a = dict(A, **over)
  p = lambda k: ctypes.c_void_p(a[k]) if a[k] is not None else None
  a.setdefault('scale', None)
  a.setdefault('shift', None)
  args = (p('gout'), p('y'), p('out'), p('vec'), p('vec'), p('vec'), p('scale'), p('shift'), 1, p('gy'), p('gadd'), p('vec'), p('vec'), 0, p('ws'), B, C, S, groups)
  return lib.mode_bn_train_bwd_amax(*args, p('vec2'), None) if amax else lib.mode_bn_train_bwd(*args, None)


def test_entries_refuse_what_the_kernels_cannot_read():
  """Every (B, C, S) tensor and the workspace, moved by 4 bytes with rows of whole 16-byte pieces and by 2 bytes with other rows: -2
  (unsupported) with the 'unaligned buffer' message, on the plain and the `_amax` entries.  And the size and pairing contracts: -1 / -2
  with their messages.  All on the host, before any launch."""
  lib = mode_hip.lib()
  for S, off in ((64, 4), (64, 8), (7, 2), (7, 1)):
    for amax in (False, True):
      for k in ('y', 'add', 'out', 'ws'):
        assert _fwd_call(lib, S, amax=amax, **{k: A[k] + off}) == -2 and b'mode_bn_train_fwd: unaligned buffer' in lib.mode_last_error(), (S, off, k)
      for k in ('gout', 'y', 'out', 'gy', 'gadd', 'ws'):
        assert _bwd_call(lib, S, amax=amax, **{k: A[k] + off}) == -2 and b'mode_bn_train_bwd: unaligned buffer' in lib.mode_last_error(), (S, off, k)
    for k in ('y', 'add', 'out'):
      assert _eval_call(lib, S, **{k: A[k] + off}) == -2 and b'mode_bn_eval_fwd: unaligned buffer' in lib.mode_last_error(), (S, off, k)
  # rows that are no whole 16-byte pieces are read element by element: 4-byte alignment is enough for them, but never for the workspace
  assert _fwd_call(lib, 7, ws=A['ws'] + 4) == -2 and b'unaligned buffer' in lib.mode_last_error()
  assert _bwd_call(lib, 7, ws=A['ws'] + 4) == -2 and b'unaligned buffer' in lib.mode_last_error()
  # B * C = 65536: one block row per (sample, channel) in a 16-bit grid dimension
  assert _fwd_call(lib, 64, B=256, C=256) == -2 and b'exceeds the grid limit' in lib.mode_last_error()
  assert _eval_call(lib, 64, B=256, C=256) == -2 and b'exceeds the grid limit' in lib.mode_last_error()
  assert _bwd_call(lib, 64, B=256, C=256) == -2 and b'exceeds the grid limit' in lib.mode_last_error()
  # groups that do not divide the batch
  assert _fwd_call(lib, 64, B=4, groups=3) == -1 and b'not divisible into 3 groups' in lib.mode_last_error()
  assert _bwd_call(lib, 64, B=4, groups=3) == -1 and b'not divisible into 3 groups' in lib.mode_last_error()
  assert _fwd_call(lib, 64, B=4, groups=0) == -1
  # in place
  assert _fwd_call(lib, 64, out=A['y']) == -1 and b'in-place operation (out == y)' in lib.mode_last_error()
  assert _bwd_call(lib, 64, gy=A['y']) == -1 and b'in-place operation (gy == y)' in lib.mode_last_error()
  # running statistics and coefficients come in pairs
  assert _fwd_call(lib, 64, rm=None) == -1 and b'running stats must come in pairs' in lib.mode_last_error()
  assert _fwd_call(lib, 64, rv=None) == -1 and b'running stats must come in pairs' in lib.mode_last_error()
  assert _fwd_call(lib, 64, scale=None) == -1 and b'save_scale / save_shift come in pairs' in lib.mode_last_error()
  assert _fwd_call(lib, 64, shift=None) == -1 and b'save_scale / save_shift come in pairs' in lib.mode_last_error()
  assert _bwd_call(lib, 64, scale=A['vec']) == -1 and b'save_scale / save_shift come in pairs' in lib.mode_last_error()
  assert _bwd_call(lib, 64, shift=A['vec']) == -1 and b'save_scale / save_shift come in pairs' in lib.mode_last_error()


# ------------------------------------------------------------------------------------------------ a tensor that really is misaligned
@gpu
@pytest.mark.parametrize('training', [True, False])
def test_bn_act_on_a_view_one_element_into_a_buffer(training):
  """y, add and the incoming gradient are contiguous views that start 4 bytes into their buffers, with rows of whole 16-byte pieces: the
  kernels cannot read them where they are.  models.stage3d.bn_act gives the bits of the call on aligned copies."""
  from models import stage3d
  shape = (2, 3, 4, 8, 33)  # S = 1056
  n = int(np.prod(shape))

  def inside(seed, scale=1.0, shift=0.0):
    flat = torch.empty(n + 1, device=DEV)
    flat[1:] = (R._rand((n,), seed, scale) + shift).to(DEV)
    v = flat[1:].view(shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v

  results = []
  for misaligned in (True, False):
    y, add, gout = inside(91, 2.0, 1.5), inside(92), inside(93)
    if not misaligned:
      y, add, gout = y.clone(), add.clone(), gout.clone()
      assert y.data_ptr() % 16 == 0
    bn = nn.BatchNorm3d(3).to(DEV).train(training)
    y.requires_grad_(training)
    add.requires_grad_(training)
    out = stage3d.bn_act(bn, y, add, relu=True)
    got = [out.detach()]
    if training:
      out.backward(gout)
      got += [y.grad, add.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var]
    results.append(got)
  for a, b in zip(*results):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
