"""GPU (-m gpu): mode_hip.optim.Adam (mode-2022_amd/mode_hip/optim.py, csrc/optim.hip) against torch.optim.Adam -- the reference's optimizer,
train_disparity.py:293: optim.Adam(params, lr, betas=(0.9, 0.999)).

Shapes: seven parameter tensors with 1, 3, 5, 864, 4097, 4098 and 1000 elements in two groups (the first four, the last three) with
different learning rates and weight decays: unaligned flat offsets from the second tensor on, a tensor smaller than a vector, and two
tensors of two whole chunks (MODE_ADAM_CHUNK = 2048 elements) plus a tail of 1 and of 2.  Values 0.05 * randn; gradients seeded per step
with the per-tensor scales 1, 1e-3, 1e-8, 1e-3, 1e-5, 10, 1e-3 (the 1e-8 tensor puts sqrt(v) next to eps).

The E rule.  torch.optim.Adam(foreach=False) runs the same steps on the CPU in float64 and in float32.  After every step and for each of
p, exp_avg and exp_avg_sq, E_ref is the largest |fp32 - fp64| over ALL elements of all tensors (a one-element tensor's own difference can be
zero by chance), E_hip the same for this optimizer against float64, and E_hip <= 2 E_ref is required: the factor is for a square root or a
division that rounds differently, not room for another formula.  The kernel forms every element operation by operation as torch does
(no FMA contraction, IEEE square root and division); the ratios are printed per step."""
import functools

import pytest
import torch

import mode_hip
from mode_hip import data_parallel, optim
from mode_hip.graph_step import GraphedStep

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIZES = [1, 3, 5, 864, 4097, 4098, 1000]
SCALES = [1, 1e-3, 1e-8, 1e-3, 1e-5, 10, 1e-3]
SPLIT = 4  # the first four tensors are group 0
LRS = (1e-3, 3e-3)
N = sum(SIZES)


def _values():
  g = torch.Generator().manual_seed(20221)
  return [0.05 * torch.randn(n, generator=g) for n in SIZES]


@functools.lru_cache(maxsize=None)
def _grads(step):
  g = torch.Generator().manual_seed(7000 + step)
  return tuple(s * torch.randn(n, generator=g) for n, s in zip(SIZES, SCALES))


def _groups(params, wd, **more):
  return [dict(params=params[:SPLIT], lr=LRS[0], weight_decay=wd, **more), dict(params=params[SPLIT:], lr=LRS[1], weight_decay=wd / 2, **more)]


def _cat(ts):
  return torch.cat([t.detach().reshape(-1).double().cpu() for t in ts])


def _torch_state(opt, params):
  return (_cat(params), _cat([opt.state[p]['exp_avg'] for p in params]), _cat([opt.state[p]['exp_avg_sq'] for p in params]))


@functools.lru_cache(maxsize=None)
def _torch_run(dtype, wd, steps, max_norm=None):
  """[(p, exp_avg, exp_avg_sq) after step k] of torch.optim.Adam(foreach=False) on the CPU in `dtype` (all as float64 vectors); computed once
  per configuration and shared between the tests."""
  params = [torch.nn.Parameter(v.to(dtype)) for v in _values()]
  opt = torch.optim.Adam(_groups(params, wd), betas=(0.9, 0.999), foreach=False)
  out = []
  for k in range(steps):
    for p, g in zip(params, _grads(k)):
      p.grad = g.clone().to(dtype)  # (a copy: clip_grad_norm_ scales .grad in place, and _grads is shared)
    if max_norm is not None:
      torch.nn.utils.clip_grad_norm_(params, max_norm)
    opt.step()
    out.append(_torch_state(opt, params))
  return out


def _ours(wd=0.0, **kw):
  params = [torch.nn.Parameter(v.to(DEV)) for v in _values()]
  return params, optim.Adam(_groups(params, wd), betas=(0.9, 0.999), **kw)


def _load(opt, k):
  opt.flat.copy_(torch.cat(_grads(k)).to(DEV))


def _state(params, opt):
  return (_cat(params), opt.exp_avg.double().cpu(), opt.exp_avg_sq.double().cpu())


def _bits(params, opt):
  return [torch.cat([p.detach().reshape(-1) for p in params]).clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()]


def _same_bits(a, b):
  return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _e_rule(tag, k, got, ref32, ref64):
  ratios = []
  for name, g, a, b in zip(('p', 'exp_avg', 'exp_avg_sq'), got, ref32, ref64):
    e_ref, e_hip = float((a - b).abs().max()), float((g - b).abs().max())
    ratios.append(e_hip / e_ref if e_ref > 0 else float('inf') if e_hip > 0 else 0.0)
    print('%s step %d %-10s E_hip %.3e  E_ref %.3e  ratio %.3f' % (tag, k + 1, name, e_hip, e_ref, ratios[-1]))
  for name, g, a, b in zip(('p', 'exp_avg', 'exp_avg_sq'), got, ref32, ref64):
    e_ref, e_hip = float((a - b).abs().max()), float((g - b).abs().max())
    assert e_hip <= 2 * e_ref, (tag, k + 1, name, e_hip, e_ref)
  return ratios


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize('wd', [0.0, 1e-2])
def test_six_steps_follow_torchs_adam(wd):
  ref64, ref32 = _torch_run(torch.float64, wd, 6), _torch_run(torch.float32, wd, 6)
  params, opt = _ours(wd)
  worst = 0.0
  for k in range(6):
    _load(opt, k)
    opt.step()
    worst = max([worst] + _e_rule('wd=%g' % wd, k, _state(params, opt), ref32[k], ref64[k]))
  print('wd=%g: worst ratio E_hip / E_ref over six steps %.3f' % (wd, worst))
  assert float(opt.step_count) == 6 and float(opt.skipped_steps) == 0 and float(opt.found_inf) == 0


# ------------------------------------------------------------------------------------------------ 2. bits
def _eager(steps, wd=1e-2, lr_at=None, **kw):
  params, opt = _ours(wd, **kw)
  for k in range(steps):
    if k == lr_at:
      opt.param_groups[0]['lr'] = 5e-4
    _load(opt, k)
    opt.step()
  torch.cuda.synchronize()
  return params, opt


def test_two_fresh_optimizers_end_with_the_same_bits():
  a, b = _eager(3), _eager(3)
  assert _same_bits(_bits(*a), _bits(*b))
  assert float(a[1].grad_norm) == float(b[1].grad_norm)


def _captured(wd=1e-2):
  """A fresh optimizer and a torch.cuda.graph capture of its step() (the code objects are loaded by the eager runs of the caller)."""
  params, opt = _ours(wd)
  graph = torch.cuda.CUDAGraph()
  torch.cuda.synchronize()
  with torch.cuda.graph(graph):
    opt.step()
  return params, opt, graph


def test_three_replays_of_a_captured_step_equal_three_eager_steps():
  want = _bits(*_eager(3))
  params, opt, graph = _captured()
  assert float(opt.step_count) == 0  # a capture runs nothing
  for k in range(3):
    _load(opt, k)  # into the same buffer, between the replays
    graph.replay()
  torch.cuda.synchronize()
  assert _same_bits(_bits(params, opt), want)
  assert float(opt.step_count) == 3


def test_a_learning_rate_change_reaches_a_captured_step_through_sync_hyperparameters():
  p_e, o_e = _eager(3, lr_at=2)
  assert not _same_bits(_bits(p_e, o_e)[:1], _bits(*_eager(3))[:1])  # (the change matters)
  params, opt, graph = _captured()
  for k in range(3):
    if k == 2:
      opt.param_groups[0]['lr'] = 5e-4
      assert opt.sync_hyperparameters() is True and opt.sync_hyperparameters() is False  # one copy, and only when something changed
    _load(opt, k)
    graph.replay()
  torch.cuda.synchronize()
  assert _same_bits(_bits(params, opt), _bits(p_e, o_e))


# ------------------------------------------------------------------------------------------------ 3. guard
@pytest.mark.parametrize('where,bad', [(N - 1, float('inf')), (0, float('nan'))])
def test_a_non_finite_gradient_skips_the_step(where, bad):
  params, opt = _eager(2)
  twin_p, twin = _eager(2)
  before = _bits(params, opt)
  _load(opt, 2)
  opt.flat[where] = bad
  opt.step()
  torch.cuda.synchronize()
  assert _same_bits(_bits(params, opt), before), 'a skipped step wrote something'
  assert float(opt.step_count) == 2 and float(opt.found_inf) == 1 and float(opt.skipped_steps) == 1
  # the following finite step: as if the bad one had never been seen
  for o in (opt, twin):
    _load(o, 3)
    o.step()
  torch.cuda.synchronize()
  assert _same_bits(_bits(params, opt), _bits(twin_p, twin))
  assert float(opt.step_count) == 3 == float(twin.step_count) and float(opt.found_inf) == 0 and float(opt.skipped_steps) == 1
  assert float(twin.skipped_steps) == 0
  # the switch is the guard: without it the same input poisons the state
  p_off, o_off = _eager(2, skip_nonfinite=False)
  _load(o_off, 2)
  o_off.flat[where] = bad
  o_off.step()
  torch.cuda.synchronize()
  assert float(o_off.step_count) == 3 and float(o_off.found_inf) == 1 and float(o_off.skipped_steps) == 0
  assert bool(torch.isnan(o_off.exp_avg_sq).any()) or bool(torch.isinf(o_off.exp_avg_sq).any())
  assert any(bool(torch.isnan(p).any()) for p in p_off)


# ------------------------------------------------------------------------------------------------ 4. norm
def test_the_gradient_norm_is_the_float64_norm():
  """Fewer than 2^14 elements, squares exact in fp64, each fp64 addition at most 2^-53 relative: the sum is good to about 1.8e-12; the
  rest of 1e-11 is room for the square root and the fold order."""
  params, opt = _ours()
  for k in range(2):
    _load(opt, k)
    opt.step()
    want = float(torch.cat(_grads(k)).double().norm())
    got = float(opt.grad_norm)
    print('step %d: grad_norm %.17g  float64 %.17g  relative difference %.3e' % (k + 1, got, want, abs(got - want) / want))
    assert abs(got - want) <= 1e-11 * want


# ------------------------------------------------------------------------------------------------ 5. clipping
def test_clipping_follows_clip_grad_norm_and_leaves_the_gradient_alone():
  max_norm = 0.5 * float(torch.cat(_grads(0)).double().norm())
  ref64, ref32 = _torch_run(torch.float64, 0.0, 6, max_norm), _torch_run(torch.float32, 0.0, 6, max_norm)
  plain = _torch_run(torch.float32, 0.0, 1)
  assert not torch.equal(plain[0][1], ref32[0][1])  # (the clip is active)
  params, opt = _ours(0.0, max_grad_norm=max_norm)
  for k in range(6):
    _load(opt, k)
    opt.step()
    _e_rule('clip', k, _state(params, opt), ref32[k], ref64[k])
    # unlike torch.nn.utils.clip_grad_norm_, which scales .grad in place, the coefficient is applied on the fly
    assert torch.equal(opt.flat.cpu(), torch.cat(_grads(k)))
    assert abs(float(opt.grad_norm) - 2 * max_norm) <= 1e-11 * 2 * max_norm or k > 0  # the norm reported is the one before clipping


# ------------------------------------------------------------------------------------------------ 6. torch sees the writes
def test_the_version_counters_move_eagerly_and_in_a_replay():
  params, opt = _ours()
  _load(opt, 0)
  v0 = [p._version for p in params]
  opt.step()
  assert all(p._version > v for p, v in zip(params, v0))

  def fn():
    opt.step()
    return opt.grad_norm

  graphed = GraphedStep(fn, warmup=1)
  assert {id(p) for p in params} <= {id(t) for t in graphed.written}
  v1 = [p._version for p in params]
  before = float(opt.step_count)
  graphed.replay()
  torch.cuda.synchronize()
  assert all(p._version > v for p, v in zip(params, v1))
  assert float(opt.step_count) == before + 1


# ------------------------------------------------------------------------------------------------ 7. state interchange
def test_state_dict_has_torchs_keys_and_shapes():
  params = [torch.nn.Parameter(v.view(-1, 1).to(DEV)) for v in _values()]  # (n, 1): the shapes are the parameters', not flat
  frozen = torch.nn.Parameter(torch.zeros(7, device=DEV), requires_grad=False)
  assert optim.Adam(_groups(params, 0.0)).state_dict()['state'] == {}  # like torch: nothing before the first step
  opt = optim.Adam(_groups(params[:2] + [frozen] + params[2:], 1e-2), betas=(0.9, 0.999))  # (takes the .grad views over)
  for k in range(2):
    _load(opt, k)
    opt.step()
  cpu = [torch.nn.Parameter(p.detach().cpu().clone()) for p in params[:2] + [frozen] + params[2:]]
  cpu[2].requires_grad_(False)
  theirs = torch.optim.Adam(_groups(cpu, 1e-2), betas=(0.9, 0.999), foreach=False)
  for p, g in zip(cpu[:2] + cpu[3:], _grads(0)):
    p.grad = g.view(-1, 1)
  theirs.step()
  a, b = opt.state_dict(), theirs.state_dict()
  assert sorted(a) == sorted(b) == ['param_groups', 'state']
  assert sorted(a['state']) == sorted(b['state']) == [0, 1, 3, 4, 5, 6, 7]  # torch's numbering; the frozen parameter (2) has no state
  for i in a['state']:
    assert list(a['state'][i]) == list(b['state'][i]) == ['step', 'exp_avg', 'exp_avg_sq']
    for key in a['state'][i]:
      x, y = a['state'][i][key], b['state'][i][key]
      assert x.shape == y.shape and x.dtype == y.dtype, (i, key, x.shape, y.shape)
    assert float(a['state'][i]['step']) == 2
  assert [g['params'] for g in a['param_groups']] == [g['params'] for g in b['param_groups']]
  assert all(set(gb) <= set(ga) and ga['lr'] == gb['lr'] and ga['betas'] == gb['betas'] for ga, gb in zip(a['param_groups'], b['param_groups']))


def test_a_run_changes_optimizer_in_both_directions():
  wd = 1e-2
  ref64, ref32 = _torch_run(torch.float64, wd, 4), _torch_run(torch.float32, wd, 4)
  # ours for two steps, then torch's on cloned parameters
  params, opt = _eager(2, wd)
  cpu = [torch.nn.Parameter(p.detach().cpu().clone()) for p in params]
  theirs = torch.optim.Adam(_groups(cpu, wd), betas=(0.9, 0.999), foreach=False)
  theirs.load_state_dict(opt.state_dict())
  for k in (2, 3):
    for p, g in zip(cpu, _grads(k)):
      p.grad = g.clone()
    theirs.step()
    _e_rule('ours -> torch', k, _torch_state(theirs, cpu), ref32[k], ref64[k])
  # torch's for two steps (the fp32 run itself, stepped again here to have its state_dict), then ours
  cpu = [torch.nn.Parameter(v.clone()) for v in _values()]
  theirs = torch.optim.Adam(_groups(cpu, wd), betas=(0.9, 0.999), foreach=False)
  for k in (0, 1):
    for p, g in zip(cpu, _grads(k)):
      p.grad = g.clone()
    theirs.step()
  params, opt = _ours(wd)
  with torch.no_grad():
    for p, q in zip(params, cpu):
      p.copy_(q)
  opt.load_state_dict(theirs.state_dict())
  assert float(opt.step_count) == 2
  for k in (2, 3):
    _load(opt, k)
    opt.step()
    _e_rule('torch -> ours', k, _state(params, opt), ref32[k], ref64[k])
  # steps that differ inside the saved state are refused: one counter serves all
  sd = theirs.state_dict()
  sd['state'][3]['step'] = torch.tensor(5.0)
  with pytest.raises(ValueError, match='step'):
    opt.load_state_dict(sd)
  sd['state'][3]['step'] = 2.0  # a float, as older checkpoints hold it
  for i in sd['state']:
    sd['state'][i]['step'] = 2.0
  opt.load_state_dict(sd)
  assert float(opt.step_count) == 2


# ------------------------------------------------------------------------------------------------ the views
def test_zero_grad_keeps_the_views_and_step_notices_a_lost_one():
  params, opt = _ours()
  _load(opt, 0)
  addr = [p.grad.data_ptr() for p in params]
  assert addr == [opt.flat.data_ptr() + 4 * sum(SIZES[:i]) for i in range(len(SIZES))]
  for arg in (True, False):
    opt.zero_grad(set_to_none=arg)
    assert [p.grad.data_ptr() for p in params] == addr and not bool(opt.flat.any())
    _load(opt, 0)
  torch.optim.Optimizer.zero_grad(opt, set_to_none=True)  # what a foreign zero_grad does
  assert params[0].grad is None
  with pytest.raises(RuntimeError, match=r'zero_grad\(\) of THIS optimizer'):
    opt.step()
  assert float(opt.step_count) == 0
  opt.zero_grad()
  assert [p.grad.data_ptr() for p in params] == addr
  _load(opt, 0)
  opt.step()
  assert float(opt.step_count) == 1
  # step(closure): the closure runs with gradients enabled and its value comes back
  assert opt.step(lambda: 1.5) == 1.5 and float(opt.step_count) == 2
  with pytest.raises(ValueError, match='fixed at construction'):
    opt.add_param_group({'params': [torch.nn.Parameter(torch.zeros(3, device=DEV))]})


def test_adopting_a_reducers_buffer_is_checked_by_address():
  net = torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.Linear(3, 2)).to(DEV)
  reducer = data_parallel.GradAllReducer(net, fuse_accumulation=False)
  opt = optim.Adam(net.parameters(), lr=1e-3, flat_grads=reducer.flat)
  assert opt.flat is reducer.flat and opt.numel == 5 * 3 + 3 + 3 * 2 + 2
  with pytest.raises(ValueError, match='parameter order'):
    optim.Adam(list(net.parameters())[::-1], flat_grads=reducer.flat)
  with pytest.raises(ValueError, match='flat_grads'):
    optim.Adam(net.parameters(), flat_grads=reducer.flat[:-1])
  net(torch.ones(4, 5, device=DEV)).sum().backward()
  opt.step()
  assert float(opt.step_count) == 1 and float(opt.grad_norm) == pytest.approx(float(reducer.flat.double().norm()), rel=1e-11)


# ------------------------------------------------------------------------------------------------ 8. the trajectory the reference walked
@pytest.mark.parametrize('how', ['whole_step_graph', 'eager_update'])
def test_three_training_steps_follow_the_reference(golden, how):
  """The third variant of tests/test_gpu_steps.py::test_three_training_steps_follow_the_reference: the same golden file, helpers and bounds,
  with mode_hip.optim.Adam on the reducer's flat buffer -- the whole step (zero-grad, forward, loss, backward, update) as ONE GraphedStep, or
  the update run eagerly after the replay."""
  import test_gpu_steps as S
  z = golden('model_steps_tiny.npz')
  net, left, right, gt, K = S._setup(z)
  net.train()
  p0 = {k: v.detach().cpu().double().clone() for k, v in net.named_parameters()}
  count = data_parallel.global_valid_count(~torch.isnan(gt))
  reducer = data_parallel.GradAllReducer(net)
  opt = optim.Adam(net.parameters(), lr=S.LR, betas=(0.9, 0.999), flat_grads=reducer.flat)
  # the capture's warm-up runs the body: BatchNorm state moves, and with the update inside also the parameters and the optimizer state
  state = {k: v.detach().clone() for k, v in net.state_dict().items()}
  fresh = opt.state_dict()

  def body():
    opt.zero_grad()
    loss, _ = net.forward_loss(left, right, gt, count=count)
    loss.backward()
    if how == 'whole_step_graph':
      opt.step()
    return loss

  graphed = GraphedStep(body, (left, right, gt, count), warmup=1)
  with torch.no_grad():
    for k, v in net.state_dict().items():
      v.copy_(state[k])
  opt.load_state_dict(fresh)
  assert float(opt.step_count) == 0
  losses = []
  for _ in range(K):
    loss = graphed.replay()
    if how == 'eager_update':
      reducer.all_reduce()
      opt.step()
    losses.append(float(loss))
  torch.cuda.synchronize()
  assert float(opt.step_count) == K and float(opt.skipped_steps) == 0
  S._check(z, net, p0, losses, 'own Adam, ' + how)
