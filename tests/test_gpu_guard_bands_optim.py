"""Guard bands for the optimizer entries (csrc/optim.hip: mode_adam_prepare, mode_adam_update): no read or write outside the buffers they
were given.

As tests/test_gpu_guard_bands_spp.py: the case is registered in the operator table of tests/test_gpu_guard_bands.py
(test_gpu_guard_bands.CASES, through its own case() helper) when this module is imported -- this file sorts in front of
tests/test_guard_bands_host.py, so the ledger there sees the two entries whenever the suite is collected as a whole.  It runs here through
test_gpu_guard_bands.run_case (declared entries launched, guards intact under both fills, outputs bit-equal between the fills and finite).

The case is the seven tensors of tests/test_gpu_optim.py (1, 3, 5, 864, 4097, 4098 and 1000 elements in two groups): unaligned flat offsets
from the second tensor on, a tensor smaller than a vector, chunks with a tail of 1 and of 2 elements.  Every parameter tensor and the flat
gradient buffer are placed between guards; exp_avg, exp_avg_sq, the segment and chunk tables, the reduction's workspace and the device block
are allocations of mode_hip/optim.py, which the guard allocator relocates -- the workspace is a torch.empty, filled with a different
pattern in each of the two runs: bit equality between the fills also proves that the fold reads only columns that were written.  Two steps
with weight decay and clipping on, so that the second one reads moments that the first one wrote."""
import pytest
import torch

import test_gpu_guard_bands as T

from mode_hip import optim

ADAM_ENTRIES = ('mode_adam_prepare', 'mode_adam_update')
SIZES = (1, 3, 5, 864, 4097, 4098, 1000)
SCALES = (1, 1e-3, 1e-8, 1e-3, 1e-5, 10, 1e-3)
HYPER = (dict(lr=1e-3, weight_decay=1e-2), dict(lr=3e-3, weight_decay=5e-3))
MAX_NORM = 100.0  # (the norm of these gradients is about 640: the clip is active)


def _tensors(sizes):
  values = [0.05 * T._rand((n,), 100 + i) for i, n in enumerate(sizes)]
  grads = [[T._rand((n,), 200 + 10 * k + i, s) for i, (n, s) in enumerate(zip(sizes, SCALES))] for k in range(2)]
  return values, grads


def b_adam(*sizes):
  values, grads = _tensors(sizes)

  def run():
    params = [torch.nn.Parameter(T.P(v)) for v in values]
    flat = T.P(torch.cat(grads[0]))
    off = 0
    for p in params:  # what data_parallel.GradAllReducer does: .grad as views of the flat buffer
      p.grad = flat[off:off + p.numel()].view_as(p)
      off += p.numel()
    opt = optim.Adam([dict(params=params[:4], **HYPER[0]), dict(params=params[4:], **HYPER[1])], betas=(0.9, 0.999), flat_grads=flat,
                     max_grad_norm=MAX_NORM)
    norms = []
    for k in range(2):
      flat.copy_(torch.cat(grads[k]))
      opt.step()
      norms.append(opt.grad_norm.clone())
    out = {'p%d' % i: p.detach() for i, p in enumerate(params)}
    out.update(exp_avg=opt.exp_avg, exp_avg_sq=opt.exp_avg_sq, norm0=norms[0], norm1=norms[1], step=opt.step_count.clone(),
               skipped=opt.skipped_steps.clone(), flat=flat)
    return out

  def verify(out):
    ref = [torch.nn.Parameter(v.double()) for v in values]
    theirs = torch.optim.Adam([dict(params=ref[:4], **HYPER[0]), dict(params=ref[4:], **HYPER[1])], betas=(0.9, 0.999), foreach=False)
    for k in range(2):
      for p, g in zip(ref, grads[k]):
        p.grad = g.double()
      norm = torch.nn.utils.clip_grad_norm_(ref, MAX_NORM)
      assert abs(float(out['norm%d' % k]) - float(norm)) <= 1e-11 * float(norm)
      theirs.step()
    # (the optimizer's own bound is the E rule of tests/test_gpu_optim.py; here: the right numbers at all -- an update moves an entry by ~lr)
    for i, p in enumerate(ref):
      T.close(out, 'p%d' % i, p.detach(), 1e-6)
    T.close(out, 'exp_avg', torch.cat([theirs.state[p]['exp_avg'] for p in ref]), 1e-6)
    T.close(out, 'exp_avg_sq', torch.cat([theirs.state[p]['exp_avg_sq'] for p in ref]), 1e-6)
    assert float(out['step']) == 2 and float(out['skipped']) == 0
    assert torch.equal(out['flat'], torch.cat(grads[1]))  # the gradient buffer is read, never written

  return run, verify


_FIRST = len(T.CASES)
T.case('adam', list(ADAM_ENTRIES), b_adam, SIZES)
CASES = T.CASES[_FIRST:_FIRST + 1]


def test_the_case_declares_the_optimizer_entries():
  """CPU tier.  Together with the rest of the table it covers the launching ABI (the ledger of tests/test_guard_bands_host.py)."""
  assert set().union(*[c.entries for c in CASES]) == set(ADAM_ENTRIES)
  assert all(c in T.CASES for c in CASES) and len({c.id for c in T.CASES}) == len(T.CASES)
  import test_guard_bands_host as G
  assert set(ADAM_ENTRIES) <= G.launching_entries() and set(ADAM_ENTRIES) <= G._declared_entries()
  import mode_hip
  new = {n for n in mode_hip.SIGNATURES if n.startswith('mode_adam_')}
  assert new & G.launching_entries() == set(ADAM_ENTRIES)  # exactly the new launching entries; the other two are size queries


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
def test_guarded_adam(c, monkeypatch, stop_at_a_gpu_fault):
  rec, stats = T.run_case(c, monkeypatch)
  assert c.entries, 'every case declares the entries it is there to launch'
  missing = sorted(c.entries - set(rec.launched))
  assert not missing, 'declared but not launched: %s (launched: %s)' % (missing, sorted(rec.launched))
  assert set(rec.launched) <= set(ADAM_ENTRIES), sorted(rec.launched)
  assert rec.launched['mode_adam_prepare'] == 4 and rec.launched['mode_adam_update'] == 4  # two steps under each fill
  T.STATS['allocations'] += sum(stats['allocations'])
  T.STATS['launches'] += sum(rec.launched.values())
  T.STATS['cases'] += 1
  print('  %d guarded allocations, %d launching calls' % (sum(stats['allocations']), sum(rec.launched.values())))
  print('LAUNCHED %s %s' % (c.id, ' '.join(sorted(rec.launched))))
