"""Guard bands for the spatial pyramid pooling entries (csrc/spp.hip: mode_spp_pool_fwd / _bwd, mode_spp_concat_fwd / _bwd): no read
or write outside the buffers they were given.

As tests/test_gpu_guard_bands_handoff.py: the case is registered in the operator table of tests/test_gpu_guard_bands.py
(test_gpu_guard_bands.CASES, through its own case() helper) when this module is imported, so the ledger of
tests/test_guard_bands_host.py sees the four entries whenever the suite is collected as a whole.  It runs here through
test_gpu_guard_bands.run_case (declared entries launched, guards intact under both fills, outputs bit-equal between the fills and
finite).

The case is the (72, 136) shape of tests/test_gpu_spp.py (N = 2, channels 3 / 8 / 4): floor cropping in both axes -- the second row and the third column of
64 x 64 regions hold 8 rows / 8 columns only, 9 x 17 blocks at k = 8 against 4 x 8 at k = 16 -- and the last pixel of every level's
gradient gathers up to the plane's last row and column.  raw, skip, the four branch tensors, the upstream gradient of
the concatenation and those of the four pooled tensors are all placed between guards.  Every output is a torch.empty of the host code,
which the guard allocator fills with a different pattern in each of the two runs: bit equality between the fills also proves that
every element is written."""
import pytest
import torch

import test_gpu_guard_bands as T

import test_gpu_spp as S
from mode_hip import functional as HF

SPP_ENTRIES = ('mode_spp_pool_fwd', 'mode_spp_pool_bwd', 'mode_spp_concat_fwd', 'mode_spp_concat_bwd')
SHAPE = (72, 136)


def b_spp(H, W):
  t = S._inputs(H, W)
  names = ['b%d' % k for k in S.KS]

  def run():
    T._fresh_caches()
    out = {}
    # the pooling alone: its backward gets the four pooled gradients from between guards, and no slice
    skip = T.P(t['skip']).requires_grad_(True)
    ps = HF.spp_pool(skip)
    torch.autograd.backward(list(ps), [T.P(t['gp%d' % k]) for k in S.KS])
    out.update({'pool%d' % k: p.detach() for p, k in zip(ps, S.KS)})
    out['pool/g_skip'] = skip.grad
    # the concatenation alone: every operand and the upstream gradient between guards
    leaf = {k: T.P(t[k]).requires_grad_(True) for k in ['raw', 'skip'] + names}
    cat = HF.spp_concat(leaf['raw'], leaf['skip'], *[leaf[k] for k in names])
    cat.backward(T.P(t['gcat']))
    out['cat'] = cat.detach()
    out.update({'concat/g_' + k: v.grad for k, v in leaf.items()})
    # the block without its convolutions: skip's gradient in one pass (the slice of gcat read in place + the four block gradients)
    raw, skip = T.P(t['raw']).requires_grad_(True), T.P(t['skip']).requires_grad_(True)
    ps = HF.spp_pool(skip)
    cat = HF.spp_concat(raw, ps.skip, *[p[:, :S.CB].contiguous() for p in ps])
    cat.backward(T.P(t['gcat']))
    out['block/cat'] = cat.detach()
    out['block/g_raw'], out['block/g_skip'] = raw.grad, skip.grad
    return out

  def verify(out):
    pool, concat, block = [S._truth(H, W, what) for what in S.WHAT]
    # (the kernels' own bound is that of tests/test_gpu_spp.py, relative to torch's fp32 operators; here: the right numbers at all)
    for k in S.KS:
      T.close(out, 'pool%d' % k, pool['pool%d' % k], 1e-5)
    T.close(out, 'pool/g_skip', pool['g_skip'], 1e-5)
    T.close(out, 'cat', concat['cat'], 1e-5)
    for k in ['raw', 'skip'] + names:
      T.close(out, 'concat/g_' + k, concat['g_' + k], 1e-5)
    T.close(out, 'block/cat', block['cat'], 1e-5)
    T.close(out, 'block/g_raw', block['g_raw'], 1e-5)
    T.close(out, 'block/g_skip', block['g_skip'], 1e-5)

  return run, verify


_FIRST = len(T.CASES)
T.case('spp', list(SPP_ENTRIES), b_spp, SHAPE)
CASES = T.CASES[_FIRST:_FIRST + 1]


def test_the_case_declares_the_spp_entries():
  """CPU tier.  Together with the rest of the table it covers the launching ABI (the ledger of tests/test_guard_bands_host.py)."""
  assert set().union(*[c.entries for c in CASES]) == set(SPP_ENTRIES)
  assert all(c in T.CASES for c in CASES) and len({c.id for c in T.CASES}) == len(T.CASES)
  import test_guard_bands_host as G
  assert set(SPP_ENTRIES) <= G.launching_entries() and set(SPP_ENTRIES) <= G._declared_entries()


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
def test_guarded_spp(c, monkeypatch, stop_at_a_gpu_fault):
  rec, stats = T.run_case(c, monkeypatch)
  assert c.entries, 'every case declares the entries it is there to launch'
  missing = sorted(c.entries - set(rec.launched))
  assert not missing, 'declared but not launched: %s (launched: %s)' % (missing, sorted(rec.launched))
  assert set(rec.launched) <= set(SPP_ENTRIES), sorted(rec.launched)
  assert rec.launched['mode_spp_pool_bwd'] >= 4 and rec.launched['mode_spp_concat_bwd'] >= 4  # two calls under each fill
  T.STATS['allocations'] += sum(stats['allocations'])
  T.STATS['launches'] += sum(rec.launched.values())
  T.STATS['cases'] += 1
  print('  %d guarded allocations, %d launching calls' % (sum(stats['allocations']), sum(rec.launched.values())))
  print('LAUNCHED %s %s' % (c.id, ' '.join(sorted(rec.launched))))
