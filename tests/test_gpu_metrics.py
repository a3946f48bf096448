"""GPU: utils.evaluation and the fused SILog loss (csrc/metrics.hip) against the reference's utils/evaluation.py (golden vectors of
tests/golden/make_golden_metrics.py), against float64 evaluations of the same per-element fp32 terms, against torch's own comparisons,
and in a ModeFusion training step."""
import builtins
import json

import numpy as np
import pytest
import torch

import recipe
from oracle import fusion_ref

DEV = 'cuda:0'


def _ulp(x):
  return float(np.spacing(np.abs(np.float32(x))))


def _truth64(fn, p, g):
  """float64 evaluation of the per-element fp32 terms torch forms (None where torch would raise)."""
  with np.errstate(all='ignore'):
    d = (p - g).astype(np.float32)
    e = np.abs(d)
    pos, both = g > 0, (g > 0) & (p > 0)

    def mean(t):
      return np.float64('nan') if t.size == 0 else t.astype(np.float64).sum() / t.size

    if fn == 'mae':
      return mean(e)
    if fn == 'rmse':
      return np.sqrt(mean((d * d).astype(np.float32)))
    if fn == 'absrel':
      return mean((e[pos] / g[pos]).astype(np.float32))
    if fn == 'sqrel':
      return mean(((d[pos] * d[pos]).astype(np.float32) / (g[pos] * g[pos]).astype(np.float32)).astype(np.float32))
    if fn == 'silog':
      l = np.log(p[both].astype(np.float64)) - np.log(g[both].astype(np.float64))
      return np.sqrt(mean(l * l) - mean(l) ** 2)
  raise KeyError(fn)


def _same_or_close(ours, truth, tol):
  if np.isnan(truth) or np.isinf(truth):
    return (np.isnan(ours) and np.isnan(truth)) or ours == truth
  return abs(float(ours) - float(truth)) <= tol


@pytest.mark.gpu
def test_gpu_golden_parity_of_all_ten_functions(golden):
  from utils import evaluation as E
  z = golden('metrics.npz')
  calls = json.loads(str(z['calls']))
  assert {c['fn'] for c in calls} == set(E.__all__) - {'disparity_metrics', 'depth_metrics'}
  for c in calls:
    p32, g32 = z[c['case'] + '/pred'], z[c['case'] + '/gt']
    p, g = torch.from_numpy(p32).to(DEV), torch.from_numpy(g32).to(DEV)
    what = '%s %s%s' % (c['case'], c['fn'], tuple(c['args']))
    f = getattr(E, c['fn'])
    if 'raises' in c:
      with pytest.raises(getattr(builtins, c['raises'])):
        f(*c['args'], p, g)
      continue
    v = f(*c['args'], p, g)
    ref = z[c['key']]
    assert type(v).__name__ == c['type'], what
    if c['type'] == 'float':  # percentages: counts exactly, the same Python arithmetic
      assert v == float(ref), (what, v, float(ref))
      continue
    assert v.dtype == np.dtype(c['dtype']) and list(v.shape) == c['shape'], what
    ours, ref32 = float(v), float(ref)
    if c['fn'] == 'max_ae':
      assert (np.isnan(ours) and np.isnan(ref32)) or ours == ref32, (what, ours, ref32)
      continue
    truth = _truth64(c['fn'], p32, g32)
    if c['fn'] == 'silog':
      with np.errstate(all='ignore'):
        both = (g32 > 0) & (p32 > 0)
        l = np.log(p32[both].astype(np.float64)) - np.log(g32[both].astype(np.float64))
        scale = np.sqrt((l * l).mean()) if l.size else 0.0
      tol = max(1e-6 * abs(truth), 1e-6 * scale, _ulp(truth)) if np.isfinite(truth) else 0
    else:
      tol = 2 * _ulp(truth) if np.isfinite(truth) else 0
    assert _same_or_close(ours, truth, tol), (what, ours, truth)
    # the reference's own fp32 value, within its own distance from the float64 evaluation
    if np.isfinite(truth):
      assert abs(ours - ref32) <= abs(ref32 - truth) + tol, (what, ours, ref32, truth)
    else:
      assert _same_or_close(ours, ref32, 0), (what, ours, ref32)


def _big(seed, shape=(8, 1, 1024, 512)):
  g = torch.Generator(device='cpu').manual_seed(seed)
  gt = torch.rand(shape, generator=g) * 60
  pred = gt * (1 + 0.3 * torch.randn(shape, generator=g))
  for t in (gt, pred):
    flat = t.view(-1)
    idx = torch.randint(0, flat.numel(), (3000,), generator=g)
    flat[idx[:1000]] = float('nan')
    flat[idx[1000:1500]] = float('inf')
    flat[idx[1500:2000]] = -float('inf')
    flat[idx[2000:]] = 0
  return pred, gt


@pytest.mark.gpu
def test_gpu_fused_entries_equal_the_compacted_calls_and_torch_counts():
  from utils import evaluation as E
  pred, gt = _big(5)
  pred, gt = pred.to(DEV), gt.to(DEV).squeeze(1)  # (B, 1, H, W) against (B, H, W), as the scripts call it
  mask = torch.isfinite(gt) & torch.isfinite(pred.squeeze(1)) & (gt <= 55)
  for fused, per in ((E.disparity_metrics, [E.mae, E.rmse, lambda p, g: E.pixel_error_pct(1, p, g), lambda p, g: E.pixel_error_pct(3, p, g),
                                            lambda p, g: E.pixel_error_pct(5, p, g), lambda p, g: E.D1(3, 0.05, p, g)]),
                     (E.depth_metrics, [E.mae, E.rmse, E.absrel, E.sqrel, E.silog, lambda p, g: E.delta_acc(1, p, g),
                                        lambda p, g: E.delta_acc(2, p, g), lambda p, g: E.delta_acc(3, p, g)])):
    got = fused(pred, gt, mask)
    pm, gm = pred.squeeze(1)[mask], gt[mask]
    want = [f(pm, gm) for f in per]
    assert len(got) == len(want)
    for a, b in zip(got, want):
      assert type(a) is type(b)
      if isinstance(a, float):
        assert a == b
      else:
        assert a.dtype == np.float32 and abs(float(a) - float(b)) <= _ulp(b), (float(a), float(b))
  # counts against torch's own comparisons on the GPU, with NaN / inf everywhere and no mask
  p, g = pred.view(-1), gt.view(-1)
  n = p.numel()
  e = (p - g).abs()
  r = torch.max(p / g, g / p)
  want = [100 * int((e >= t).sum()) / n for t in (1, 3, 5)] + [100 * int(((e >= 3) * (e >= 0.05 * g)).sum()) / n]
  want += [100 * int((r < 1.25**k).sum()) / n for k in (1, 2, 3)]
  got = [E.pixel_error_pct(t, p, g) for t in (1, 3, 5)] + [E.D1(th_pixel=3, th_pct=0.05, pred=p, gt=g)]
  got += [E.delta_acc(k, p, g) for k in (1, 2, 3)]
  assert got == want
  assert np.isnan(float(E.mae(p, g))) and np.isnan(float(E.max_ae(p, g)))


@pytest.mark.gpu
def test_gpu_odd_sizes_and_unaligned_slices():
  """n % 4 != 0 and bases off the 16-byte grid take the element-wise path: same counts as CPU torch, the same bits as an aligned copy."""
  from mode_hip import functional as HF
  from utils import evaluation as E
  pred, gt = _big(6, (3, 1, 77, 129))
  p, g = pred.view(-1).to(DEV), gt.view(-1).to(DEV)
  n = p.numel() - 6  # odd
  ps, gs = p[1:1 + n], g[3:3 + n]  # 4- and 12-byte offsets
  assert ps.data_ptr() % 16 and gs.data_ptr() % 16 and n % 4
  m = (torch.arange(n, device=DEV) % 7) != 3
  ms = torch.cat([torch.zeros(1, dtype=torch.bool, device=DEV), m])[1:]  # a mask at an odd byte
  a = HF.masked_metrics(ps, gs, ms, px=(1, 3), d1=((3, 0.05),), ratio=(1.25,))
  b = HF.masked_metrics(ps.clone(), gs.clone(), m.clone(), px=(1, 3), d1=((3, 0.05),), ratio=(1.25,))
  assert a.tobytes() == b.tobytes()
  pc, gc = ps.cpu()[m.cpu()], gs.cpu()[m.cpu()]
  e = (pc - gc).abs()
  assert E.pixel_error_pct(3, ps[m], gs[m]) == 100 * int((e >= 3).sum()) / pc.numel()
  assert E.delta_acc(1, ps[m], gs[m]) == 100 * int((torch.max(pc / gc, gc / pc) < 1.25).sum()) / pc.numel()
  import mode_hip
  assert a[mode_hip.M_N] == pc.numel() and a[mode_hip.M_N_GT] == int((gc > 0).sum()) and a[mode_hip.M_N_BOTH] == int(((gc > 0) & (pc > 0)).sum())


@pytest.mark.gpu
def test_gpu_metrics_are_bit_identical_across_calls_and_streams():
  from mode_hip import functional as HF
  pred, gt = _big(7)
  p, g = pred.to(DEV), gt.to(DEV)
  finite = torch.isfinite(p) & torch.isfinite(g)
  args = dict(px=(1, 3, 5), d1=((3, 0.05),), ratio=(1.25, 1.5625, 1.953125))
  a = HF.masked_metrics(p, g, finite, **args)
  b = HF.masked_metrics(p, g, finite, **args)
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(s):
    c = HF.masked_metrics(p, g, finite, **args)
  torch.cuda.synchronize()
  assert a.tobytes() == b.tobytes() == c.tobytes()
  assert np.isfinite(a).all() and a[0] == int(finite.sum())


def _loss_case(seed, B=2, H=48, W=40, maxdepth=50.0):
  g = torch.Generator(device='cpu').manual_seed(seed)
  gt = torch.rand(B, H, W, generator=g) * maxdepth * 1.2
  pred = (gt.unsqueeze(1) * (1 + 0.2 * torch.randn(B, 1, H, W, generator=g))).contiguous()
  pred.view(-1)[::37] = 0
  pred.view(-1)[5::41] = -1
  gt.view(-1)[::53] = 0
  return pred, gt, maxdepth


@pytest.mark.gpu
def test_gpu_silog_loss_matches_float64_autograd():
  from mode_hip import functional as HF
  pred, gt, maxdepth = _loss_case(11)
  p = pred.to(DEV).requires_grad_()
  g = gt.to(DEV)
  loss = HF.silog_loss(p, g, g <= maxdepth)
  loss.backward()
  p64 = pred.double().requires_grad_()
  ref = fusion_ref.training_loss(p64, gt.double(), maxdepth)
  ref.backward()
  assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
  assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-6 * abs(float(ref.detach()))
  gp, gr = p.grad.double().cpu(), p64.grad
  assert float((gp - gr).norm() / gr.norm()) <= 1e-6
  sel = ((gt <= maxdepth) & (gt > 0)).unsqueeze(1) & (pred > 0)
  assert bool((gp[~sel] == 0).all()) and bool((gp[sel] != 0).any())


@pytest.mark.gpu
def test_gpu_silog_loss_golden_cases(golden):
  """silog_loss on every case of the metric fixture (NaN, +-inf, zeros, negatives, threshold corners, empty) against the reference's
  fp32 loss stored there and a float64 evaluation of the same selection: NaN where the reference is NaN, otherwise as close to float64
  as 1e-6 relative and no farther from the reference than the reference is from float64."""
  from mode_hip import functional as HF
  z = golden('metrics.npz')
  cases = sorted(k[len('loss/'):] for k in z.files if k.startswith('loss/'))
  assert set(cases) == {'finite', 'specials', 'signed', 'boundary', 'zeros', 'empty'}
  for case in cases:
    p32, g32 = z[case + '/pred'], z[case + '/gt']
    ref32 = float(z['loss/' + case])
    ours = float(HF.silog_loss(torch.from_numpy(p32).to(DEV), torch.from_numpy(g32).to(DEV)))
    with np.errstate(all='ignore'):
      both = (g32 > 0) & (p32 > 0)
      l = np.log(p32[both].astype(np.float64)) - np.log(g32[both].astype(np.float64))
      truth = (l * l).mean() - 0.5 * l.mean() ** 2 if l.size else np.nan
    if np.isnan(ref32):
      assert np.isnan(ours) and np.isnan(truth), (case, ours, truth)
      continue
    tol = 1e-6 * max(abs(truth), (l * l).mean())
    assert abs(ours - truth) <= tol, (case, ours, truth)
    assert abs(ours - ref32) <= abs(ref32 - truth) + tol, (case, ours, ref32, truth)


@pytest.mark.gpu
def test_gpu_silog_loss_of_an_empty_selection():
  from mode_hip import functional as HF
  pred, gt, maxdepth = _loss_case(12)
  p = pred.to(DEV).requires_grad_()
  g = gt.to(DEV)
  loss = HF.silog_loss(p, g, g > 1e9)
  loss.backward()
  assert torch.isnan(loss) and bool((p.grad == 0).all())
  p64 = pred.double().requires_grad_()
  ref = fusion_ref.silog_loss(0.5, p64[:, 0][gt > 1e9], gt.double()[gt > 1e9])
  ref.backward()
  assert torch.isnan(ref) and bool((p64.grad == 0).all())  # what torch does


@pytest.mark.gpu
def test_gpu_silog_loss_graph_replay_is_eager_bit_for_bit():
  """Forward + backward of silog_loss captured into one hipGraph (mode_hip.graph_step.GraphedStep, as the training step is) and
  replayed: the eager step's bits, on every replay, and new data is picked up through the static inputs."""
  from mode_hip import functional as HF
  from mode_hip.graph_step import GraphedStep
  pred, gt, maxdepth = _loss_case(13)
  p = pred.to(DEV).requires_grad_()
  g = gt.to(DEV)

  def body():
    p.grad = None
    loss = HF.silog_loss(p, g, g <= maxdepth)
    loss.backward()
    return loss, p.grad

  eager_loss, eager_gp = [t.detach().clone() for t in body()]
  gs = GraphedStep(body, (g,), warmup=1)
  for _ in range(3):
    loss, gp = gs.replay()
    torch.cuda.synchronize()
    assert loss.detach().cpu().numpy().tobytes() == eager_loss.cpu().numpy().tobytes()
    assert gp.cpu().numpy().tobytes() == eager_gp.cpu().numpy().tobytes()
  g2 = torch.roll(g, 7, 2)
  gs.load(g2)
  loss2 = float(gs.replay()[0].detach())
  g.copy_(g2)
  assert loss2 == float(body()[0].detach()) and loss2 != float(eager_loss)


@pytest.mark.gpu
def test_gpu_fusion_training_step_with_the_fused_loss(golden):
  """tests/test_fusion.py::test_gpu_fusion_train_and_eval's training step with silog_loss in place of the torch formula: the same loss
  and parameter gradients, within that test's tolerances, against the golden vectors and against the torch-loss step."""
  from models import mode_fusion
  from mode_hip import functional as HF
  from mode_hip import no_vendor
  z = golden('fusion_tiny.npz')
  cfg = z['cfg']
  maxdepth, B, H, W, seed = float(cfg[0]), int(cfg[1]), int(cfg[2]), int(cfg[3]), int(cfg[4])
  channels = [int(c) for c in cfg[5:]]
  manifest = [(k, tuple(s)) for k, s in json.loads(str(z['manifest']))]
  rs = np.random.RandomState(seed + 1)
  depthes = [torch.from_numpy((rs.rand(B, 1, H, W) * maxdepth).astype(np.float32)).to(DEV) for _ in range(6)]
  confs = [torch.from_numpy(rs.rand(B, 1, H, W).astype(np.float32)).to(DEV) for _ in range(6)]
  rgbs = [torch.from_numpy(rs.rand(B, 3, H, W).astype(np.float32)).to(DEV) for _ in range(4)]
  gt = torch.from_numpy((rs.rand(B, H, W) * maxdepth * 1.1).astype(np.float32)).to(DEV)
  net = mode_fusion.ModeFusion(maxdepth, channels, {'depth': 12, 'rgb': 12}).to(DEV)
  net.load_state_dict(recipe.recipe_state(manifest, seed))
  net.train()
  params = dict(net.named_parameters())
  with no_vendor.no_vendor_arithmetic() as guard:
    pred = net(depthes, confs, rgbs)
    loss = HF.silog_loss(pred, gt, gt <= maxdepth)
    grads = torch.autograd.grad(loss, list(params.values()), retain_graph=True, allow_unused=True)
  assert guard.seen > 0
  assert abs(float(loss) - float(z['train/loss'])) < 1e-4 * float(z['train/loss'])
  ref_loss = fusion_ref.training_loss(pred, gt, maxdepth)
  ref_grads = torch.autograd.grad(ref_loss, list(params.values()), allow_unused=True)
  assert abs(float(loss) - float(ref_loss)) <= 1e-5 * abs(float(ref_loss))
  ours = dict(zip(params, grads))
  theirs = dict(zip(params, ref_grads))
  for n, s in zip(z['train/grad_names'], z['train/grad_abs_sum']):
    a = float(ours[str(n)].double().abs().sum())
    assert abs(a - s) <= 2e-2 * s + 1e-5, n
    b = float(theirs[str(n)].double().abs().sum())
    assert abs(a - b) <= 2e-2 * b + 1e-5, n
