"""CPU tier of the self-supervised stereo loss: the float64 restatement of tests/photometric_ref.py is a well-defined
function (its autograd gradient agrees with central differences, its window count with a brute-force count), and the C entries and
the Python entries refuse on the host what they cannot run."""
import ctypes

import pytest
import torch

import photometric_ref as R

import mode_hip
import models
from mode_hip import functional as HF


@pytest.mark.parametrize('case', R.CASES, ids=['x'.join(str(v) for v in c) for c in R.CASES])
def test_float64_restatement_against_central_differences(case):
  """Four probed elements per case (16 over the cases), taken where the gradient is largest in each quarter of map 0 and of the last
  map.  Central differences with eps = 1e-6 in float64: the truncation error is O(eps^2); each of the two evaluations of a loss of
  order 1 (sums of thousands of terms) carries a rounding error of up to ~10 ulp = 2e-15, which the quotient turns into
  2 x 2e-15 / 2e-6 = 2e-9.  Hence 2e-9 absolute + 1e-6 of max|g|; a wrong derivative (max|g| is 1e-4 .. 1e-3) misses that by orders of
  magnitude."""
  left, right, disps = R.make_case(*case)
  K = len(disps)
  loss, stats, grads = R.reference(case, torch.float64)
  assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(g).all()) for g in grads)
  eps = 1e-6
  for k in sorted({0, K - 1}):
    g = grads[k].flatten()
    n = g.numel()
    probes = [int(g[q * n // 4:(q + 1) * n // 4].abs().argmax()) + q * n // 4 for q in range(4)][:4 if K == 1 else 2]
    for i in probes:
      vals = []
      for s in (1, -1):
        ds = [d.double().clone() for d in disps]
        ds[k].view(-1)[i] += s * eps
        vals.append(float(R.photometric_loss(left, right, ds, R.WEIGHTS[:K])[0]))
      fd = (vals[0] - vals[1]) / (2 * eps)
      assert abs(fd - float(g[i])) <= 1e-6 * float(g.abs().max()) + 2e-9, (k, i, fd, float(g[i]))


@pytest.mark.parametrize('case', R.CASES[:3], ids=['x'.join(str(v) for v in c) for c in R.CASES[:3]])
def test_valid_window_count_equals_a_brute_force_count(case):
  left, right, disps = R.make_case(*case)
  _, stats, _ = R.reference(case, torch.float64)
  B, H, W = disps[0].shape
  for k, d in enumerate(disps):
    n = R.brute_force_count(left, right, d)
    assert int(stats[k, 0]) == n
    assert 0.3 * B * H * (W - 2) < n < 0.7 * B * H * (W - 2), n  # the generator leaves about half of the windows valid


def test_float32_restatement_is_close_to_float64():
  """The yardstick of the GPU parity test: the restatement's own float32 error is small and not zero."""
  for case in R.CASES:
    l64, s64, g64 = R.reference(case, torch.float64)
    l32, s32, g32 = R.reference(case, torch.float32)
    assert torch.equal(s32[:, 0].double(), s64[:, 0])
    assert 0 < abs(float(l32) - float(l64)) <= 1e-6 * abs(float(l64))
    for a, b in zip(g32, g64):
      assert 0 < float((a.double() - b).abs().max()) <= 1e-5 * float(b.abs().max())


def test_entries_refuse_bad_arguments_on_the_host():
  lib = mode_hip.lib()
  null, one = ctypes.c_void_p(0), ctypes.c_void_p(256)
  prm = mode_hip.PhotometricParams()
  p = ctypes.byref(prm)
  ws = lib.mode_photometric_loss_workspace_bytes(3, 2, 40, 24)
  assert ws > 0 and ws % 16 == 0
  assert lib.mode_photometric_loss_workspace_bytes(3, 12, 1024, 512) % 16 == 0
  assert lib.mode_photometric_loss_workspace_bytes(0, 2, 40, 24) == 0 and lib.mode_photometric_loss_workspace_bytes(3, 2, 40, 2) == 0

  def fwd(left=one, right=one, disp=one, K=3, B=2, H=40, W=24, params=p, wsp=one, wsb=ws, stats=one, loss=one):
    return lib.mode_photometric_loss_fwd(left, right, disp, K, B, H, W, params, wsp, wsb, stats, loss, null)

  def bwd(left=one, right=one, disp=one, K=3, B=2, H=40, W=24, params=p, stats=one, gloss=one, gdisp=one):
    return lib.mode_photometric_loss_bwd(left, right, disp, K, B, H, W, params, stats, gloss, gdisp, null)

  for name in ('left', 'right', 'disp', 'params', 'stats', 'loss'):
    assert fwd(**{name: null}) == -1 and b'null pointer' in lib.mode_last_error(), name
  for name in ('left', 'right', 'disp', 'params', 'stats', 'gloss', 'gdisp'):
    assert bwd(**{name: null}) == -1 and b'null pointer' in lib.mode_last_error(), name
  for call in (fwd, bwd):
    for K in (0, 5):
      assert call(K=K) == -1 and b'K' in lib.mode_last_error()
    assert call(W=2) == -1 and b'at least 3' in lib.mode_last_error()
    assert call(H=2) == -1 and b'at least 3' in lib.mode_last_error()
    assert call(B=0) == -1
    assert call(B=1 << 20, H=1024, W=512) == -2 and b'2^31' in lib.mode_last_error()  # MODE_ERR_UNSUPPORTED: 32-bit indices
  assert fwd(wsp=null) == -3 and fwd(wsb=ws - 8) == -3  # MODE_ERR_WORKSPACE


def test_python_entries_refuse_what_they_cannot_run():
  left, right, disps = R.make_case(*R.CASES[0])
  with pytest.raises(NotImplementedError, match='Only support cuda tensor!'):
    HF.photometric_loss(left, right, disps, (0.5, 0.7, 1.0))
  net = models.ModeDisparity(16, 'Sphere', 64, 32, 'Cassini')
  net.eval()
  x = torch.zeros(1, 3, 64, 32)
  with pytest.raises(RuntimeError, match='training'):
    net.forward_photometric_loss(x, x)
  erp = models.ModeDisparity(16, 'Sphere', 32, 64, 'ERP')
  erp.train()
  with pytest.raises(ValueError, match='Cassini'):
    erp.forward_photometric_loss(torch.zeros(1, 3, 32, 64), torch.zeros(1, 3, 32, 64))
