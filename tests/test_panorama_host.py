"""CPU: utils.panorama and the ERP-domain scoring entries (csrc/erp_metrics.hip) -- importing the module loads nothing native, CPU
tensors and bad shapes are refused before any native call, the C entries validate their arguments on the host (no compute calls), and
ModeMultiView.evaluate keeps forward()'s contract."""
import ctypes
import subprocess
import sys

import pytest
import torch

import mode_hip
import models
from conftest import PKG, ROOT


def test_importing_panorama_loads_no_native_library():
  code = ('import sys; sys.path[:0] = [%r, %r]\n'
          'import torch, mode_hip\n'
          'from utils import panorama\n'
          'assert callable(panorama.erp_depth_metrics) and callable(panorama.bicubic_up2)\n'
          'assert sorted(panorama.__all__) == ["bicubic_up2", "erp_depth_metrics"]\n'
          'maps = open("/proc/self/maps").read()\n'
          'assert "libmode_hip" not in maps, "libmode_hip.so mapped"\n'
          'assert mode_hip._lib is None and not torch.cuda.is_initialized()\n'
          'print("ok")\n') % (ROOT, PKG)
  r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
  assert r.returncode == 0 and r.stdout.strip() == 'ok', r.stderr


def test_cpu_tensors_are_refused():
  from mode_hip import functional as HF
  from utils import geometry, panorama
  p, g = torch.rand(2, 64, 32), torch.rand(2, 64, 32)
  grid = geometry._c2e_grid(32, 64, 'cpu')
  calls = [lambda: panorama.erp_depth_metrics(p, g), lambda: panorama.erp_depth_metrics(p.unsqueeze(1), g, return_erp=True),
           lambda: panorama.erp_depth_metrics(torch.rand(2, 1, 32, 16), g, upsample=True), lambda: panorama.bicubic_up2(torch.rand(1, 1, 8, 4)),
           lambda: HF.bicubic_up2(torch.rand(1, 1, 8, 4)), lambda: HF.erp_depth_metrics(p, g, grid, 1000.)]
  for c in calls:
    with pytest.raises(NotImplementedError):
      c()


def test_bad_shapes_are_refused_before_any_native_call(monkeypatch):
  from mode_hip import functional as HF
  from utils import panorama
  for module in (mode_hip, HF):
    monkeypatch.setattr(module, 'lib', lambda: pytest.fail('native library reached'))
  g = torch.rand(2, 64, 32)
  with pytest.raises(ValueError, match='H = 2 W'):
    panorama.erp_depth_metrics(torch.rand(2, 64, 48), torch.rand(2, 64, 48))
  with pytest.raises(ValueError, match='does not fit'):
    panorama.erp_depth_metrics(torch.rand(3, 64, 32), g)  # frame counts differ
  with pytest.raises(ValueError, match='does not fit'):
    panorama.erp_depth_metrics(torch.rand(2, 1, 64, 32), g, upsample=True)  # full-size pred with upsample=True
  with pytest.raises(ValueError, match='does not fit'):
    panorama.erp_depth_metrics(torch.rand(2, 1, 32, 16), g)  # half-size pred without it
  with pytest.raises(ValueError, match='not .F, H, W.'):
    panorama.erp_depth_metrics(torch.rand(64, 32), g)
  with pytest.raises(ValueError, match='not .F, H, W.'):
    panorama.erp_depth_metrics(torch.rand(2, 2, 64, 32), g)


def test_workspace_is_one_flat_range_workspace_per_frame():
  lib = mode_hip.lib()
  for F, H, W in ((1, 64, 32), (5, 50, 25), (4, 1024, 512), (3, 4096, 2048)):
    assert lib.mode_erp_depth_metrics_workspace_bytes(F, H, W) == F * lib.mode_masked_metrics_workspace_bytes(H * W) > 0
  assert lib.mode_erp_depth_metrics_workspace_bytes(0, 64, 32) == 0
  assert lib.mode_erp_depth_metrics_workspace_bytes(-1, 64, 32) == 0 and lib.mode_erp_depth_metrics_workspace_bytes(1, 0, 32) == 0


def test_erp_entries_validate_on_the_host():
  """mode_erp_depth_metrics / mode_bicubic_up2 refuse bad arguments before any launch, with a message."""
  lib = mode_hip.lib()
  null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
  prm = mode_hip.MetricsParams()
  F, H, W = 2, 64, 32
  need = lib.mode_erp_depth_metrics_workspace_bytes(F, H, W)

  def call(pred=one, gt=one, grid=one, F=F, H=H, W=W, params=ctypes.byref(prm), ws=one, ws_bytes=need, out=one, pe=null, ge=null):
    return lib.mode_erp_depth_metrics(pred, gt, grid, F, H, W, 1000., params, ws, ws_bytes, out, pe, ge, null)

  for kw in ('pred', 'gt', 'grid', 'out'):
    assert call(**{kw: null}) == -1 and b'null pointer' in lib.mode_last_error(), kw
  assert call(params=None) == -1 and b'null pointer' in lib.mode_last_error()
  assert call(H=64, W=48) == -1 and b'H = 2 W' in lib.mode_last_error()
  assert call(H=0, W=0) == -1 and b'bad size' in lib.mode_last_error()
  assert call(H=-64, W=-32) == -1 and b'bad size' in lib.mode_last_error()
  assert call(F=-1) == -1 and b'bad size' in lib.mode_last_error()
  assert call(H=1 << 17, W=1 << 16) == -1 and b'too large' in lib.mode_last_error()
  for field in ('n_px', 'n_d1', 'n_ratio'):
    bad = mode_hip.MetricsParams()
    setattr(bad, field, mode_hip.METRICS_MAX_THRESHOLDS + 1)
    assert call(params=ctypes.byref(bad)) == -1 and b'too many thresholds' in lib.mode_last_error()
  assert call(grid=ctypes.c_void_p(20)) == -1 and b'8-byte aligned' in lib.mode_last_error()
  assert call(ws=null) == -3 and b'workspace' in lib.mode_last_error()
  assert call(ws=ctypes.c_void_p(20)) == -3 and b'workspace' in lib.mode_last_error()
  assert call(ws_bytes=need - 8) == -3 and b'too small' in lib.mode_last_error()
  assert call(F=0, pred=null, gt=null, grid=null, out=null, ws=null, ws_bytes=0) == 0  # nothing to do: no launch
  # mode_bicubic_up2
  assert lib.mode_bicubic_up2(null, one, 1, 1, 8, 4, null) == -1 and b'null pointer' in lib.mode_last_error()
  assert lib.mode_bicubic_up2(one, null, 1, 1, 8, 4, null) == -1 and b'null pointer' in lib.mode_last_error()
  assert lib.mode_bicubic_up2(one, one, 1, 1, 8, 4, null) == -1 and b'in-place' in lib.mode_last_error()
  two = ctypes.c_void_p(32)
  assert lib.mode_bicubic_up2(one, two, 1, 0, 8, 4, null) == -1 and b'non-positive size' in lib.mode_last_error()
  assert lib.mode_bicubic_up2(one, two, -1, 1, 8, 4, null) == -1 and b'non-positive size' in lib.mode_last_error()
  assert lib.mode_bicubic_up2(one, two, 1, 1, 8, 0, null) == -1 and b'non-positive size' in lib.mode_last_error()
  assert lib.mode_bicubic_up2(one, two, 1, 1, 1 << 20, 4, null) == -1 and b'too large' in lib.mode_last_error()
  assert lib.mode_bicubic_up2(null, null, 0, 1, 8, 4, null) == 0


def test_evaluate_keeps_the_contract_of_forward():
  net = models.ModeMultiView(16, 10., 64, 32, channels=(8, 16, 32, 64))
  assert net.maxdepth == 10.
  frames, gt = torch.zeros(1, 12, 3, 64, 32), torch.zeros(1, 64, 32)
  with pytest.raises(RuntimeError, match='inference only'):
    net.train().evaluate(frames, gt)
  with pytest.raises(NotImplementedError):
    net.eval().evaluate(frames, gt)
