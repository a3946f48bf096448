"""Guard bands for the 8-bit ingest entries (mode_frames_u8_ingest, mode_rgb_half_pil, mode_decimate2): no read or write outside the
buffers they were given.

tests/test_gpu_guard_bands.py holds the operator table and tests/test_guard_bands_host.py the ledger that requires a guarded case for
every launching entry of mode_hip.SIGNATURES.  The three cases below are registered in that same table (test_gpu_guard_bands.CASES,
through its own case() helper) when this module is imported, so the ledger sees them whenever the suite is collected as a whole -- as
the project's commands collect it.  Run as a single file (pytest tests/test_guard_bands_host.py), the ledger test does not import
this module and reports the three entries as undeclared.

The cases run here through test_gpu_guard_bands.run_case with the assertions of its test_guarded (declared entries launched, guards
intact under both fills, outputs bit-equal between the fills and finite), and verify the values bit for bit against the host references of
tests/ingest_ref.py.  uint8 inputs sit between integer guard fills (0x01 / 0x02 bytes): a byte fetched from a guard changes the output
between the two runs."""
import pytest
import torch

import ingest_ref as R
import test_gpu_guard_bands as T

from dataloader import gpu_ingest
from mode_hip import functional as HF

INGEST_ENTRIES = ('mode_frames_u8_ingest', 'mode_rgb_half_pil', 'mode_decimate2')


def _fresh_caches():
  """The tables of the ingest are cached per device / per size: drop them too, so that every run uploads them inside its guarded context."""
  T._fresh_caches()
  for c in (gpu_ingest._lut_cache, gpu_ingest._half_cache):
    c.d.clear()
    c.pinned.clear()


def b_frames_u8(F_, H, W):
  """tests/test_gpu_ingest.py: the ingest equals the host transform + split_frames, with and without the fusion RGB."""
  frames = R.frames_u8(F_, H, W, 31 + H)

  def run():
    _fresh_caches()
    left, right, rgb = gpu_ingest.frames_u8_gpu(T.P(torch.from_numpy(frames)))
    l2, r2, _ = gpu_ingest.frames_u8_gpu(T.P(torch.from_numpy(frames)), want_rgb=False)
    return {'left': left, 'right': right, 'rgb': rgb, 'left2': l2, 'right2': r2}

  def verify(out):
    wl, wr, wrgb = R.host_split(frames)
    assert torch.equal(out['left'], wl) and torch.equal(out['right'], wr) and torch.equal(out['rgb'], wrgb)
    assert torch.equal(out['left2'], wl) and torch.equal(out['right2'], wr)

  return run, verify


def b_rgb_half(F_, H, W):
  """tests/test_gpu_ingest.py: the 8-bit result is Pillow's, the float result the host transform of it.  The last frame's last panorama
  ends at the rear guard and frame 0's first begins at the front guard: both are panoramas the kernel reads."""
  frames = R.frames_u8(F_, H, W, 37 + H, 'binary')

  def run():
    _fresh_caches()
    rgb, u8 = gpu_ingest.rgb_half_gpu(T.P(torch.from_numpy(frames)), return_u8=True)
    return {'rgb': rgb, 'u8': u8, 'rgb_alone': gpu_ingest.rgb_half_gpu(T.P(torch.from_numpy(frames)))}

  def verify(out):
    want_u8, want = R.host_rgb_half(frames)
    assert torch.equal(out['u8'], want_u8) and torch.equal(out['rgb'], want) and torch.equal(out['rgb_alone'], want)

  return run, verify


def b_decimate2(*shape):
  x = T._rand(shape, 41 + sum(shape))

  def run():
    return {'y': HF.decimate2(T.P(x))}

  def verify(out):
    assert torch.equal(out['y'], x[..., ::2, ::2])

  return run, verify


_FIRST = len(T.CASES)
T.case('frames_u8_ingest', ['mode_frames_u8_ingest'], b_frames_u8, (2, 48, 32))
T.case('rgb_half_pil', ['mode_rgb_half_pil'], b_rgb_half, (2, 32, 16))
T.case('rgb_half_pil', ['mode_rgb_half_pil'], b_rgb_half, (2, 96, 80))
T.case('decimate2', ['mode_decimate2'], b_decimate2, (3, 6, 10))   # the scalar kernel
T.case('decimate2', ['mode_decimate2'], b_decimate2, (24, 32, 16))  # the 16-byte kernel
T.case('decimate2', ['mode_decimate2'], b_decimate2, (2, 5, 7))    # odd sizes: the last row and column are read, nothing behind them
CASES = T.CASES[_FIRST:]


def test_the_cases_declare_exactly_the_three_ingest_entries():
  """CPU tier.  Together with the existing table they cover the launching ABI (the ledger of tests/test_guard_bands_host.py)."""
  assert set().union(*[c.entries for c in CASES]) == set(INGEST_ENTRIES)
  assert all(c in T.CASES for c in CASES) and len({c.id for c in T.CASES}) == len(T.CASES)
  import test_guard_bands_host as L
  assert set(INGEST_ENTRIES) <= L.launching_entries()
  assert not L.launching_entries() - L._declared_entries()


@pytest.fixture
def stop_at_a_gpu_fault():
  """As test_gpu_guard_bands._stop_at_a_gpu_fault (not autouse here: this file has a CPU-tier test): if the device no longer answers
  after a test, the session ends there."""
  yield
  try:
    torch.cuda.synchronize()
  except RuntimeError as e:
    pytest.exit('the GPU reported an error after this test; nothing more is started on it: %s' % e, returncode=3)


@pytest.mark.gpu
@pytest.mark.parametrize('c', CASES, ids=[c.id for c in CASES])
def test_guarded_ingest(c, monkeypatch, stop_at_a_gpu_fault):
  rec, stats = T.run_case(c, monkeypatch)
  assert c.entries, 'every case declares the entries it is there to launch'
  missing = sorted(c.entries - set(rec.launched))
  assert not missing, 'declared but not launched: %s (launched: %s)' % (missing, sorted(rec.launched))
  assert set(rec.launched) <= set(INGEST_ENTRIES), sorted(rec.launched)
  T.STATS['allocations'] += sum(stats['allocations'])
  T.STATS['launches'] += sum(rec.launched.values())
  T.STATS['cases'] += 1
  print('  %d guarded allocations, %d launching calls' % (sum(stats['allocations']), sum(rec.launched.values())))
  print('LAUNCHED %s %s' % (c.id, ' '.join(sorted(rec.launched))))
