"""CPU: utils.evaluation and the fused SILog loss -- the reference's scripts resolve their imports on our packages, the metric functions
keep the reference's signatures, importing them loads nothing native, CPU tensors are refused, and the C entries of csrc/metrics.hip
validate their arguments on the host (no compute calls)."""
import ctypes
import importlib
import json
import os
import subprocess
import sys

import pytest
import torch

import mode_hip
from conftest import GOLDEN, PKG, ROOT


def _manifest():
  with open(os.path.join(GOLDEN, 'script_imports.json')) as f:
    return json.load(f)


def test_reference_script_imports_resolve_on_our_packages():
  """Every `from models|utils|dataloader... import ...` of the reference's top-level scripts (test_disparity.py:23-25,
  train_disparity.py:23-27, train_fusion.py:14-17, test_fusion.py:8-21, save_output_disparity_stage.py:9-12) finds its name here."""
  rows = _manifest()['imports']
  assert {r['script'] for r in rows} >= {'test_disparity.py', 'train_disparity.py', 'train_fusion.py', 'test_fusion.py',
                                         'save_output_disparity_stage.py'}
  missing = []
  for r in rows:
    mod = importlib.import_module(r['module'])
    assert os.path.realpath(mod.__file__).startswith(os.path.realpath(PKG)), (r['module'], mod.__file__)
    for name in r['names']:
      if not hasattr(mod, name):
        try:
          importlib.import_module(r['module'] + '.' + name)
        except ImportError:
          missing.append('%s:%d from %s import %s' % (r['script'], r['line'], r['module'], name))
  assert not missing, missing


def test_evaluation_signatures_are_the_references():
  from utils import evaluation
  import inspect
  for fn, params in _manifest()['evaluation_signatures'].items():
    sig = inspect.signature(getattr(evaluation, fn))
    got = [[k, None if p.default is inspect.Parameter.empty else repr(p.default)] for k, p in sig.parameters.items()]
    assert got == params, fn


def test_importing_evaluation_loads_no_native_library():
  """Forked DataLoader workers and the CPU tier import utils.evaluation: no libmode_hip.so, no GPU runtime initialised."""
  code = ('import sys; sys.path[:0] = [%r, %r]\n'
          'import torch, mode_hip\n'
          'from utils import evaluation\n'
          'from mode_hip import functional\n'
          'maps = open("/proc/self/maps").read()\n'
          'assert "libmode_hip" not in maps, "libmode_hip.so mapped"\n'
          'assert mode_hip._lib is None and not torch.cuda.is_initialized()\n'
          'print("ok")\n') % (ROOT, PKG)
  r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
  assert r.returncode == 0 and r.stdout.strip() == 'ok', r.stderr


def test_cpu_tensors_are_refused():
  from utils import evaluation as E
  from mode_hip import functional as HF
  p, g = torch.rand(16), torch.rand(16)
  m = torch.ones(16, dtype=torch.bool)
  calls = [lambda: E.mae(p, g), lambda: E.max_ae(p, g), lambda: E.rmse(p, g), lambda: E.absrel(p, g), lambda: E.sqrel(p, g),
           lambda: E.silog(p, g), lambda: E.pixel_error_pct(3, p, g), lambda: E.D1(th_pixel=3, th_pct=0.05, pred=p, gt=g),
           lambda: E.delta_acc(1, p, g), lambda: E.threshold_acc(0.25, p, g), lambda: E.disparity_metrics(p, g, m),
           lambda: E.depth_metrics(p, g, m), lambda: HF.silog_loss(p.requires_grad_(), g, m)]
  for c in calls:
    with pytest.raises(NotImplementedError):
      c()


def test_metric_entries_validate_on_the_host():
  """mode_masked_metrics / mode_silog_loss_fwd / _bwd refuse bad arguments before any launch, with a message."""
  lib = mode_hip.lib()
  null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
  n = 1000
  need = lib.mode_masked_metrics_workspace_bytes(n)
  assert need >= mode_hip.METRICS_COUNT * 8 and need % 8 == 0
  assert lib.mode_masked_metrics_workspace_bytes(-1) == 0
  prm = mode_hip.MetricsParams()
  P = ctypes.byref(prm)
  assert lib.mode_masked_metrics(null, one, null, n, P, one, need, one, null) == -1 and b'null pointer' in lib.mode_last_error()
  assert lib.mode_masked_metrics(one, one, null, n, None, one, need, one, null) == -1 and b'null pointer' in lib.mode_last_error()
  assert lib.mode_masked_metrics(one, one, null, n, P, one, need, null, null) == -1 and b'null pointer' in lib.mode_last_error()
  assert lib.mode_masked_metrics(one, one, null, -5, P, one, need, one, null) == -1 and b'negative size' in lib.mode_last_error()
  for field in ('n_px', 'n_d1', 'n_ratio'):
    bad = mode_hip.MetricsParams()
    setattr(bad, field, mode_hip.METRICS_MAX_THRESHOLDS + 1)
    assert lib.mode_masked_metrics(one, one, null, n, ctypes.byref(bad), one, need, one, null) == -1
    assert b'too many thresholds' in lib.mode_last_error()
  assert lib.mode_masked_metrics(one, one, null, n, P, one, need - 8, one, null) == -3 and b'too small' in lib.mode_last_error()
  assert lib.mode_masked_metrics(one, one, null, n, P, null, need, one, null) == -3 and b'workspace' in lib.mode_last_error()
  assert lib.mode_silog_loss_fwd(one, null, null, n, 0.5, one, need, one, one, null) == -1 and b'null pointer' in lib.mode_last_error()
  assert lib.mode_silog_loss_fwd(one, one, null, n, 0.5, one, need, one, null, null) == -1 and b'null pointer' in lib.mode_last_error()
  assert lib.mode_silog_loss_fwd(one, one, null, -1, 0.5, one, need, one, one, null) == -1 and b'negative size' in lib.mode_last_error()
  assert lib.mode_silog_loss_fwd(one, one, null, n, 0.5, one, 0, one, one, null) == -3 and b'too small' in lib.mode_last_error()
  assert lib.mode_silog_loss_bwd(one, one, null, n, 0.5, null, one, one, null) == -1 and b'null pointer' in lib.mode_last_error()
  assert lib.mode_silog_loss_bwd(one, one, null, n, 0.5, one, one, null, null) == -1 and b'null pointer' in lib.mode_last_error()
  assert lib.mode_silog_loss_bwd(one, one, null, -2, 0.5, one, one, one, null) == -1 and b'negative size' in lib.mode_last_error()
