"""GPU (-m gpu): every form of the windowed spherical kernels against the float64 oracle on tables of other sizes than the 256 x 128 one
the rest of the suite pins them on -- 192 x 96, 162 x 81, 72 x 36, 200 x 100, 512 x 256 -- and on a perturbed 192 x 96 table, which is not
shift-invariant along its rows and takes the paths a Cassini table never does (no polar items: the pixel-list fallback; an adjoint plan
that is mostly six-source tiles).

Order of every case: the numpy interpreter of tests/sphere_plan_ref.py first checks the plans the kernels are about to be given (the
device table's own), and a case fails there, before any launch, if a plan is inconsistent.  The float64 oracle
(oracle/sphere_conv_ref.py forward / backward) is computed once per (table, channels) and shared.  SPHERE_FWD_MIN_WG and
SPHERE_BWD_SPLIT_MIN_WG are 0, so that the small tables run the windowed kernels too.

Bounds, from the project's own tests of the same operators (errors are printed beside them):
  forward, fp32 window and eval epilogue   2e-6 (ci / groups * 9) max(1, |y|max)            tests/test_gpu_kernels.py
  input gradient                           2e-6 (co / groups * 9) max(1, |gx|max)           tests/test_gpu_split.py
  weight gradient                          1e-5 max(1, |gw|max)                             tests/test_gpu_split.py
  forward on bf16 / fp16 pieces            2^-22 sqrt(9 ci / groups) |y|max                 tests/test_gpu_f16.py
Every output is pre-filled with NaN (or, where the operator adds, is checked to be finite), a second call gives the same bits, and the
entries that ran are the expected ones (the recorder of tests/test_gpu_size_contracts.py)."""
import zlib

import numpy as np
import pytest
import torch

import cpu_threads
import mode_hip
import sphere_plan_ref as R
import sphere_tables as T
from mode_hip import functional as HF
from oracle import sphere_conv_ref
from test_gpu_size_contracts import RecordingLib

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

TABLES = {
    '192x96': lambda: T.geometric(96, 192),
    '162x81': lambda: T.geometric(81, 162),
    '72x36': lambda: T.geometric(36, 72),
    '200x100': lambda: T.geometric(100, 200),
    'perturbed 192x96': T.perturbed,
    '512x256': lambda: T.geometric(256, 512),
}
NO_ADJPLAN = ('162x81', '72x36', '200x100')  # H is not a multiple of 64
SPLIT_CHANNELS = [(16, 16, 1), (32, 48, 2)]
F32_CHANNELS = SPLIT_CHANNELS + [(8, 12, 1)]


def _cases(channels, extra=()):
  out = []
  for name in TABLES:
    for ch in ([(16, 16, 1)] if name == '512x256' else list(channels) + list(extra)):
      out.append(pytest.param(name, ch, id='%s-%d-%d-g%d' % ((name.replace(' ', '_'),) + ch)))
  return out


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
  assert torch.cuda.is_available(), 'GPU tests need a GPU'
  mode_hip.lib()


@pytest.fixture(autouse=True)
def _switches(monkeypatch):
  monkeypatch.setattr(HF, 'SPHERE_FWD_MIN_WG', 0)
  monkeypatch.setattr(HF, 'SPHERE_BWD_SPLIT_MIN_WG', 0)
  keep = (HF.CONV_ARITH, HF.SPHERE_FWD_F16, HF.SPHERE_BWD_F16, HF.SPHERE_BWD_DATA_SPLIT, HF.SPHERE_BWD_WEIGHT_SPLIT, HF.SPHERE_POLAR)
  yield
  HF.set_conv_arith(keep[0])
  HF.SPHERE_FWD_F16, HF.SPHERE_BWD_F16, HF.SPHERE_BWD_DATA_SPLIT, HF.SPHERE_BWD_WEIGHT_SPLIT, HF.SPHERE_POLAR = keep[1:]


@pytest.fixture
def recorder(monkeypatch):
  real = mode_hip.lib()
  proxy = RecordingLib(real)
  monkeypatch.setattr(mode_hip, '_lib', proxy)
  yield proxy
  monkeypatch.setattr(mode_hip, '_lib', real)


def _ran(recorder, prefix='mode_sphere_conv_'):
  names = [n for n in recorder.names if n.startswith(prefix)]
  del recorder.names[:]
  return names


_DEVICE_TABLES = {}  # name -> (table, its device copy, plan, adjoint plan) | the PlanError of its check; the plan caches key on the table's address
_ORACLE = {}


def _table(name):
  """The device copy of table `name` with its plans, checked by the interpreter -- before anything is launched on them."""
  if name not in _DEVICE_TABLES:
    host = TABLES[name]()
    pd = host.to(DEV)
    plan, aplan = HF.sphere_plan(pd, 3, 3), HF.sphere_adjplan(pd, 3, 3)
    try:
      assert plan is not None, 'no plan for table %s' % name
      assert (aplan is None) == (name in NO_ADJPLAN), name
      out = R.check_plan(host, plan, aplan)
      print('table %s: the plans are consistent (sampling error %.3e, bound %.3e)' % ((name,) + out['sample']))
      _DEVICE_TABLES[name] = (host, pd, plan, aplan)
    except AssertionError as e:
      _DEVICE_TABLES[name] = e
  hit = _DEVICE_TABLES[name]
  if isinstance(hit, AssertionError):
    raise hit
  return hit


def _oracle(name, ch):
  """Inputs and float64 results of (table, channels), computed once: B = 2 (1 at 512 x 256)."""
  key = (name, ch)
  if key not in _ORACLE:
    ci, co, groups = ch
    host = TABLES[name]()
    H, W = host.shape[2:]
    B = 1 if name == '512x256' else 2
    r = np.random.RandomState(zlib.crc32(repr(key).encode()))  # (the same data whichever cases run, in any order)
    x = torch.from_numpy(r.standard_normal((B, ci, H, W)).astype(np.float32))
    w = torch.from_numpy((r.standard_normal((co, ci // groups, 3, 3)) * (2.0 / (9 * ci // groups))**0.5).astype(np.float32))
    gy = torch.from_numpy(r.standard_normal((B, co, H, W)).astype(np.float32))
    torch.set_num_threads(cpu_threads.usable_cores())
    cfg = ((1, 1), (1, 1), (1, 1), groups)
    y = sphere_conv_ref.forward(x.double(), host, w.double(), *cfg)
    gx, gw = sphere_conv_ref.backward(x.double(), host, w.double(), gy.double(), *cfg)
    _ORACLE[key] = dict(x=x.to(DEV), w=w.to(DEV), gy=gy.to(DEV), y=y, gx=gx, gw=gw, B=B)
  return _ORACLE[key]


def _err(got, want):
  return float((got.detach().cpu().double() - want).abs().max())


def _eval_bn(C, seed):
  bn = torch.nn.BatchNorm2d(C).to(DEV).eval()
  r = np.random.RandomState(seed)
  with torch.no_grad():
    bn.weight.copy_(torch.from_numpy(r.uniform(0.5, 1.5, C).astype(np.float32)))
    bn.bias.copy_(torch.from_numpy((r.standard_normal(C) * 0.3).astype(np.float32)))
    bn.running_mean.copy_(torch.from_numpy((r.standard_normal(C) * 0.5).astype(np.float32)))
    bn.running_var.copy_(torch.from_numpy(r.uniform(0.3, 2.0, C).astype(np.float32)))
  return bn


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize('name,ch', _cases(F32_CHANNELS))
def test_forward_forms_against_float64(name, ch, recorder):
  """The fp32 window kernel, three bf16 pieces, two fp16 pieces (where the channel count has the split kernels: 16 per group) and the
  eval epilogue (relu + add) of the fp32 window kernel, through the NCHW entries."""
  host, pd, plan, aplan = _table(name)
  o = _oracle(name, ch)
  ci, co, groups = ch
  B, (H, W) = o['B'], host.shape[2:]
  ymax = float(o['y'].abs().max())
  forms = [('fp32 window', 'f32', False, 'mode_sphere_conv_fwd_win', 2e-6 * (ci // groups * 9) * max(1.0, ymax))]
  if ch in SPLIT_CHANNELS:
    bound = 2.0**-22 * np.sqrt(9 * ci // groups) * ymax
    forms += [('three bf16 pieces', 'bf16x6', False, 'mode_sphere_conv_fwd_win_split', bound),
              ('two fp16 pieces', 'bf16x6', True, 'mode_sphere_conv_fwd_win_split_f16', bound)]
  got = {}
  for form, arith, f16, entry, bound in forms:
    HF.set_conv_arith(arith)
    HF.SPHERE_FWD_F16 = True
    del recorder.names[:]
    y = HF.sphere_conv_fwd(o['x'], pd, o['w'], torch.full((B, co, H, W), float('nan'), device=DEV), (1, 1), groups, f16=f16)
    ran = _ran(recorder)
    again = HF.sphere_conv_fwd(o['x'], pd, o['w'], torch.full((B, co, H, W), float('nan'), device=DEV), (1, 1), groups, f16=f16)
    e = _err(y, o['y'])
    print('sphere_conv_fwd %s %d->%d g=%d B=%d [%s]: error %.3e, bound %.3e (max |y| %.3g)' % (name, ci, co, groups, B, form, e, bound, ymax))
    assert ran == [entry], (form, ran)
    assert torch.isfinite(y).all(), form
    assert e <= bound, (form, e, bound)
    assert torch.equal(y, again), form
    got[form] = y
  if ch in SPLIT_CHANNELS:
    assert not torch.equal(got['two fp16 pieces'], got['three bf16 pieces']), 'the fp16 kernel did not run'
  # the eval epilogue of the fp32 window kernel
  HF.set_conv_arith('f32')
  bn = _eval_bn(co, 77)
  add = torch.from_numpy(np.random.RandomState(78).standard_normal((B, co, H, W)).astype(np.float32)).to(DEV)
  with torch.no_grad():
    scale = (bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)).cpu().view(1, co, 1, 1)
    pre = (o['y'] - bn.running_mean.double().cpu().view(1, co, 1, 1)) * scale + bn.bias.double().cpu().view(1, co, 1, 1) + add.cpu().double()
  del recorder.names[:]
  with torch.no_grad():
    y = HF.sphere_conv_bn_eval(o['x'], pd, o['w'], bn, (1, 1), groups, add, True)
    ran = _ran(recorder)
    again = HF.sphere_conv_bn_eval(o['x'], pd, o['w'], bn, (1, 1), groups, add, True)
  e, bound = _err(y, torch.relu(pre)), 2e-6 * (ci // groups * 9) * max(1.0, float(pre.abs().max()))
  print('sphere_conv_bn_eval %s %d->%d g=%d B=%d [relu + add]: error %.3e, bound %.3e' % (name, ci, co, groups, B, e, bound))
  assert ran == ['mode_sphere_conv_fwd_win_bn'], ran
  assert torch.isfinite(y).all() and e <= bound, (e, bound)
  assert torch.equal(y, again)


# ------------------------------------------------------------------------------------------------ input gradient
@pytest.mark.parametrize('name,ch', _cases(SPLIT_CHANNELS, extra=[(48, 32, 2)]))
def test_input_gradient_forms_against_float64(name, ch, recorder):
  """sphere_conv_bwd_data_t with SPHERE_BWD_DATA_SPLIT on, on three bf16 pieces and on two fp16 pieces.  The windowed adjoint runs where
  the table has an adjoint plan AND the layer has 16 output channels per group (16 -> 16 and 48 -> 32 in two groups; 32 -> 48 in two
  groups has 24 and stays on the gather kernel, like the tables without an adjoint plan), the gather kernel on a tile list takes the
  plan's bad tiles."""
  host, pd, plan, aplan = _table(name)
  o = _oracle(name, ch)
  ci, co, groups = ch
  B, (H, W) = o['B'], host.shape[2:]
  windowed = aplan is not None and co // groups % 16 == 0
  assert windowed == (name not in NO_ADJPLAN and ch != (32, 48, 2))
  gyt = HF.transpose_planes(o['gy'])
  bound = 2e-6 * (co // groups * 9) * max(1.0, float(o['gx'].abs().max()))
  HF.set_conv_arith('bf16x6')
  HF.SPHERE_BWD_DATA_SPLIT = True
  got = {}
  for f16 in (False, True):
    HF.SPHERE_BWD_F16 = f16
    del recorder.names[:]
    gxt = HF.sphere_conv_bwd_data_t(gyt, pd, o['w'], torch.full((B, ci, W, H), float('nan'), device=DEV), groups)
    ran = _ran(recorder)
    again = HF.sphere_conv_bwd_data_t(gyt, pd, o['w'], torch.full((B, ci, W, H), float('nan'), device=DEV), groups)
    e = _err(gxt.transpose(2, 3), o['gx'])
    print('sphere_conv_bwd_data_t %s %d->%d g=%d B=%d [%s, %s]: error %.3e, bound %.3e (max |gx| %.3g)' %
          (name, ci, co, groups, B, 'two fp16 pieces' if f16 else 'three bf16 pieces', ', '.join(n[len('mode_sphere_conv_bwd_data_'):] for n in ran),
           e, bound, float(o['gx'].abs().max())))
    if windowed:
      want = ['mode_sphere_conv_bwd_data_win_split' + ('_f16' if f16 else '')] + (['mode_sphere_conv_bwd_data_adj_list'] if aplan.nbad else [])
    else:
      want = ['mode_sphere_conv_bwd_data_adj']
    assert ran == want, ran
    assert torch.isfinite(gxt).all()
    assert e <= bound, (f16, e, bound)
    assert torch.equal(gxt, again), 'not deterministic'
    got[f16] = gxt
  if windowed:
    assert not torch.equal(got[True], got[False]), 'the fp16 kernel did not run'
  # the NCHW operator takes the same route through the transposed copy it is handed
  HF.SPHERE_BWD_F16 = True
  gx = HF.sphere_conv_bwd_data(o['gy'], pd, o['w'], torch.full((B, ci, H, W), float('nan'), device=DEV), (1, 1), groups, overwrite=True,
                               gy_transposed=gyt)
  assert torch.equal(gx, got[True].transpose(2, 3))


# ------------------------------------------------------------------------------------------------ weight gradient
@pytest.mark.parametrize('name,ch', _cases(F32_CHANNELS))
def test_weight_gradient_forms_against_float64(name, ch, recorder):
  """sphere_conv_bwd_weight_t on the fp32 window kernels, on the split kernels and on two fp16 pieces, and the NCHW entry with the polar
  kernel and with the pixel-list fallback.  The perturbed table has no polar items: its NCHW entries take the pixel list whatever
  SPHERE_POLAR says, and the `_t` entry, which has no NCHW tensors for the general kernel, raises."""
  host, pd, plan, aplan = _table(name)
  o = _oracle(name, ch)
  ci, co, groups = ch
  B, (H, W) = o['B'], host.shape[2:]
  scale = max(1.0, float(o['gw'].abs().max()))
  bound = 1e-5 * scale
  xt, gyt = HF.transpose_planes(o['x']), HF.transpose_planes(o['gy'])
  zeros = lambda: torch.zeros((co, ci // groups, 3, 3), device=DEV)
  forms = [('fp32 window', 'f32', False, 'mode_sphere_conv_bwd_weight_win')]
  if ch in SPLIT_CHANNELS:
    forms += [('split', 'bf16x6', False, 'mode_sphere_conv_bwd_weight_win_split'),
              ('two fp16 pieces', 'bf16x6', True, 'mode_sphere_conv_bwd_weight_win_split_f16')]

  def check(form, run, entry):
    del recorder.names[:]
    gw = run()
    ran = _ran(recorder)
    again = run()
    e = _err(gw, o['gw'])
    print('sphere_conv_bwd_weight %s %d->%d g=%d B=%d [%s]: error %.3e, bound %.3e (max |gw| %.3g)' % (name, ci, co, groups, B, form, e, bound, scale))
    assert ran == [entry], (form, ran)
    assert torch.isfinite(gw).all(), form
    assert e <= bound, (form, e, bound)
    assert torch.equal(gw, again), form
    return gw

  for form, arith, f16, entry in forms:
    HF.set_conv_arith(arith)
    HF.SPHERE_BWD_F16 = f16
    if name.startswith('perturbed'):
      assert plan.polar is None and plan.nrest > 0
      del recorder.names[:]
      with pytest.raises(RuntimeError, match='pixel-list fallback'):
        HF.sphere_conv_bwd_weight_t(gyt, pd, xt, zeros(), groups)
      assert _ran(recorder) == []  # it refused before any launch
    else:
      check(form + ', plane-transposed', lambda: HF.sphere_conv_bwd_weight_t(gyt, pd, xt, zeros(), groups), entry)
    for polar in (True, False):
      HF.SPHERE_POLAR = polar
      check('%s, NCHW, %s' % (form, 'polar kernel' if (polar and plan.polar is not None) else 'pixel list'),
            lambda: HF.sphere_conv_bwd_weight(o['gy'], pd, o['x'], zeros(), (1, 1), groups), entry)
    HF.SPHERE_POLAR = True
