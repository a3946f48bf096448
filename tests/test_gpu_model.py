"""GPU (-m gpu): the drop-in ModeDisparity module on the HIP path against the golden vectors that the imported
reference produced (tests/golden/*.npz).

Tolerance.  BASELINE.json's north_star asks for 1e-3 abs on the final disparity.  On these fixtures the reference's OWN
fp32 CPU run is only reproducible to E_ref = max|reference_fp32 - fp64 evaluation| = 2e-3 (tiny) .. 1.4e-2 (config 1),
measured by tests/golden/make_golden.py and stored in the fixtures: any re-ordering of fp32 sums (MFMA tiles, split-K)
moves the result by that much, so two correct fp32 implementations cannot agree to 1e-3 there.  The bound used is
therefore on the error against truth64: mean <= 2x the reference's own mean error and max <= max(1e-3, 3 * E_ref) -- the GPU
path must be as close to the exact network as the reference itself is (see _check_disp) -- and max|gpu - reference_fp32|
is printed next to it.  Kernel-level parity (test_gpu_kernels.py)
is checked at fp32 round-off."""
import numpy as np
import pytest
import torch

import recipe
from oracle import mode_ref

import models
import mode_hip
import op_trace

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DISP_TOL = 1e-3


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
  assert torch.cuda.is_available(), 'GPU tests need a GPU'
  mode_hip.lib()


def _setup(z, bn_from_fixture=False):
  maxdisp, H, W, B, seed = [int(v) for v in z['cfg']]
  sd = recipe.recipe_state(recipe.load_manifest(), seed)
  if bn_from_fixture:
    for k in z.files:
      if k.startswith('bn/'):
        sd[k[3:]] = torch.from_numpy(z[k]).clone()
  net = models.ModeDisparity(maxdisp, 'Sphere', H, W, 'Cassini').to(DEV)
  net.load_state_dict(sd)
  left, right = recipe.recipe_images(B, H, W, seed + 1)
  gt = recipe.recipe_disparity(B, H, W, seed + 2, maxdisp)
  return net, left.to(DEV), right.to(DEV), gt.to(DEV), maxdisp


def _check_disp(name, got, ref32, truth64, e_ref, mean_floor=DISP_TOL / 10, max_factor=3.0):
  """got: HIP path; ref32: the reference's own fp32 run; truth64: fp64 evaluation of the same network.
  The error of any fp32 evaluation against truth64 is amplified round-off: its MEAN over the pixels is a stable statistic,
  its MAX is a single draw that moves by a factor of ~2 with any change of summation order (measured: 7.1e-3 and 1.65e-2
  for two equally exact kernels at config 1, 1.07e-2 for the reference itself).  Hence: mean error at most twice the
  reference's own mean error, max error at most 3x the reference's own max error (>= the north_star's 1e-3)."""
  got = got.detach().cpu().numpy().astype(np.float64)
  err = np.abs(got - truth64)
  ref_err = np.abs(np.asarray(ref32, dtype=np.float64) - truth64)
  bound_max = max(DISP_TOL, max_factor * float(e_ref))
  bound_mean = max(mean_floor, 2.0 * float(ref_err.mean()))  # (a mean error below 1e-4 px is a tenth of the north_star's bound)
  print('%s: |gpu-truth64| max %.3e mean %.3e   reference itself: max %.3e mean %.3e   |gpu-ref32| max %.3e' %
        (name, err.max(), err.mean(), ref_err.max(), ref_err.mean(), np.abs(got - ref32).max()))
  assert err.max() <= bound_max, (name, err.max(), bound_max)
  assert err.mean() <= bound_mean, (name, err.mean(), bound_mean)


def _sub(z, t):
  return t if z['train/pred1'].shape[-1] == t.shape[-1] else t[:, :, ::4, ::4]


@pytest.mark.parametrize('fixture', ['model_tiny.npz', 'model_cfg1.npz'])
def test_train_forward_backward(golden, fixture):
  z = golden(fixture)
  net, left, right, gt, maxdisp = _setup(z)
  net.train()
  preds = net(left, right)
  for i, p in enumerate(preds):
    _check_disp('%s train pred%d' % (fixture, i + 1), _sub(z, p), z['train/pred%d' % (i + 1)], z['truth64/train_pred%d' % (i + 1)],
                z['truth64/train_E_ref'])
  mask = ~torch.isnan(gt)
  loss = mode_ref.training_loss(preds, gt, mask)
  assert abs(float(loss.detach()) - float(z['train/loss'])) < 2e-4 * float(z['train/loss'])
  loss.backward()
  # Gradients: the same fp32 re-association noise is amplified by back-propagation through ~60 BatchNorm layers (the two
  # fp32 runs differ by ~1 % in sum|grad| of early-layer tensors); a wrong kernel, index map or dropped term is an O(1)
  # error.  Bounds: 5 % on sum|grad| per tensor, and at most 2 % of the sampled entries (4 per tensor) off by > 10 %.
  grads = dict(net.named_parameters())
  worst = 0.0
  for n, s in zip(z['train/grad_names'], z['train/grad_abs_sum']):
    g = grads[str(n)].grad.detach().cpu().reshape(-1).double()
    rel = abs(float(g.abs().sum()) - s) / (s + 1e-7)
    worst = max(worst, rel)
    assert rel < 5e-2, (str(n), rel)
  print('%s: worst relative error of sum|grad| over 83 weight + 160 BN tensors: %.3e' % (fixture, worst))
  bad = total = 0
  for n, s, idx, val in zip(z['train/grad_names'], z['train/grad_abs_sum'], z['train/grad_idx'], z['train/grad_val']):
    g = grads[str(n)].grad.detach().cpu().reshape(-1).double()
    scale = s / g.numel()
    bad += int((np.abs(g[idx].numpy() - val) > 0.1 * np.abs(val) + 0.1 * scale).sum())
    total += len(idx)
  print('%s: %d of %d sampled gradient entries off by more than 10 %%' % (fixture, bad, total))
  assert bad <= 0.02 * total, (bad, total)


@pytest.mark.parametrize('fixture', ['model_tiny.npz', 'model_cfg1.npz'])
def test_eval_and_confidence(golden, fixture):
  z = golden(fixture)
  net, left, right, gt, maxdisp = _setup(z, bn_from_fixture=True)
  net.eval()
  net.out_conf = True
  with torch.no_grad():
    pred, conf = net(left, right)
  _check_disp('%s eval pred3' % fixture, _sub(z, pred), z['eval/pred3'], z['truth64/eval_pred3'], z['truth64/eval_E_ref'])
  # the confidence sums 3 probabilities around round(pred): compare where the rounding is not at a tie
  ref_pred = z['eval/pred3']
  stable = np.abs(np.abs(ref_pred - np.round(ref_pred)) - 0.5) > 0.05
  diff = np.abs(_sub(z, conf).cpu().numpy() - z['eval/conf'])
  assert diff[stable].max() < 2e-2 and np.median(diff) < 1e-3
  net.out_conf = False
  with torch.no_grad():  # same answer without the confidence output (the vendor 2D convs split K with atomics: not bit-stable)
    assert (net(left, right) - pred).abs().max() < max(DISP_TOL, float(z['truth64/eval_E_ref']))


@pytest.mark.parametrize('tag', ['none', 'both'])
def test_hourglass_golden(golden, tag):
  """hourglass(4) on the HIP 3D kernels (stride-2 conv, transposed conv, skips) against the reference's own module."""
  import json
  from models.mode_disparity import hourglass
  z = golden('hourglass.npz')
  manifest = [(k, tuple(s)) for k, s in json.loads(str(z['manifest']))]
  hg = hourglass(4).to(DEV)
  hg.load_state_dict(recipe.recipe_state(manifest, 11))
  hg.train()
  x = torch.from_numpy(z['x']).to(DEV).requires_grad_(True)
  a = torch.from_numpy(z['presqu']).to(DEV) if tag == 'both' else None
  b = torch.from_numpy(z['postsqu']).to(DEV) if tag == 'both' else None
  out, pre, post = hg(x, a, b)
  for name, t in (('out', out), ('pre', pre), ('post', post)):
    assert np.abs(t.detach().cpu().numpy() - z['%s/%s' % (tag, name)]).max() < 2e-4, name
  (out * torch.from_numpy(z[tag + '/gout']).to(DEV)).sum().backward()
  assert np.abs(x.grad.cpu().numpy() - z[tag + '/gx']).max() < 5e-4
  for k, p in hg.named_parameters():
    g = z['%s/grad/%s' % (tag, k)]
    assert np.abs(p.grad.cpu().numpy() - g).max() < 1e-3 * max(1.0, np.abs(g).max()), k


def test_bench_two_ranks_share_one_gpu():
  """`python bench.py --gpus 2` with no launcher around it: bench.py itself starts one process per rank (torch.distributed.run
  as a child), flat-gradient all-reduce, barrier + max-over-ranks timing, rank 0 prints the one JSON line.  Two ranks on ONE
  GPU need the gloo backend (RCCL refuses duplicate devices); on an 8-GPU node the same path runs over RCCL."""
  import json
  import os
  import subprocess
  import sys
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
  cmd = [sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--steps', '2', '--warmup', '1', '--height', '256',
         '--width', '128', '--maxdisp', '64', '--batch', '1', '--full', '--no-cpu-baseline', '--dist-backend', 'gloo', '--value-1gpu', '10.0']
  r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
  lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
  assert r.returncode == 0 and len(lines) == 1, (r.stdout[-2000:], r.stderr[-2000:])
  d = json.loads(lines[0])
  assert d['n_gpus'] == 2 and d['config']['global_batch'] == 2 and d['value'] > 0 and d['scaling'] == 'weak'
  assert len(d['rank_ms_per_step']) == 2 and d['collective']['ranks'] == 2 and d['collective']['bytes'] == 4 * 5489280
  assert abs(d['per_gpu_value'] * 2 - d['value']) < 1e-9 * d['value']
  # the timed steps were hipGraph replays under the process group too (bench.py falls back to eager launches when capture fails,
  # and says so in this field: a silent fallback would be timed as if it were the product's launch path)
  assert d['config']['launch'].startswith('hipGraph'), d['config']['launch']
  assert d['collective']['avg_ms_rank0'] is not None and d['collective']['avg_ms_rank0'] > 0
  assert d['scaling_vs_1gpu']['value_1gpu'] == 10.0 and abs(d['scaling_vs_1gpu']['efficiency'] - d['value'] / 20.0) < 1e-12
  assert 0 < d['targets']['regulariser3d_mfma_frac'] < 1 and 0 < d['roofline']['frac'] < 1 and 0 < d['roofline']['by_label']['frac'] < 1


@pytest.mark.parametrize('mode', ['train', 'eval'])
def test_bench_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path, mode):
  """A plain `bench.py` run (no --full) times exactly --steps steps and prints the headline line without the extras; --dump-outputs
  writes what the last timed step computed -- loss, predictions, gradient buffer and state after the optimizer step for training, the
  disparity map for inference -- as float32 .npy files."""
  import json
  import os
  import subprocess
  import sys
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
  cmd = [sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--height', '256', '--width', '128',
         '--maxdisp', '64', '--batch', '1', '--mode', mode, '--dump-outputs', str(tmp_path)]
  r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
  lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
  assert r.returncode == 0 and len(lines) == 1, (r.stdout[-2000:], r.stderr[-2000:])
  d = json.loads(lines[0])
  assert d['steps'] == 3 and d['warmup'] == 1 and d['unit'] == 'pairs/s' and d['higher_is_better'] is True and d['dtype']
  assert d['metric'].startswith('ERP stereo pairs/sec') and abs(d['value'] * d['ms_per_step'] - 1e3) < 1e-6 * 1e3
  assert d['config']['launch'].startswith('hipGraph')
  assert d['roofline'] is None and d['collective'] is None and not {'cpu_baseline', 'eval_b1', 'clocks', 'kernels', 'targets'} & set(d)
  got = {f[:-4]: np.load(os.path.join(str(tmp_path), f)) for f in os.listdir(str(tmp_path))}
  want = {'loss', 'grad', 'disp1', 'disp2', 'disp3', 'state'} if mode == 'train' else {'disp'}
  assert set(got) == want and all(a.dtype == np.float32 for a in got.values())
  assert got['disp1' if mode == 'train' else 'disp'].size == 256 * 128
  if mode == 'train':
    assert all(np.isfinite(a).all() for a in got.values())
    assert got['loss'].size == 1 and got['grad'].size == 5489280 and got['state'].size > got['grad'].size and np.abs(got['grad']).max() > 0


def test_smoke_entry():
  import __graft_entry__
  __graft_entry__.smoke()


def _tiny_net(seed=3):
  torch.manual_seed(seed)
  net = models.ModeDisparity(32, 'Sphere', 128, 64, 'Cassini').to(DEV).train()
  left = torch.randn(1, 3, 128, 64, device=DEV)
  right = torch.roll(left, -3, 3) + 0.01 * torch.randn_like(left)
  gt = torch.rand(1, 1, 128, 64, device=DEV) * 14
  return net, left, right, gt


def _loss(net, left, right, gt):
  import torch.nn.functional as F
  return sum(w * F.smooth_l1_loss(o, gt) for w, o in zip((0.5, 0.7, 1.0), net(left, right)))


def test_gradient_sinks_match_autograd_accumulation():
  """GradAllReducer(fuse_accumulation=True): the native weight-gradient / BatchNorm backward kernels add straight into the
  flat gradient buffer and autograd gets None.  Same gradients as the plain autograd route, including a second backward
  on top (accumulation) and num_batches_tracked counted by the kernel."""
  from mode_hip import data_parallel
  net, left, right, gt = _tiny_net()
  _loss(net, left, right, gt).backward()
  plain = {k: p.grad.clone() for k, p in net.named_parameters()}
  nbt = {k: int(v) for k, v in net.state_dict().items() if k.endswith('num_batches_tracked')}
  assert set(nbt.values()) == {1, 2}  # the shared feature extractor sees two batches per step (left, right)
  # run-to-run noise floor of the plain route (the vendor 2D weight-gradient kernels split K with atomics)
  net.zero_grad(set_to_none=True)
  _loss(net, left, right, gt).backward()
  noise = {k: float((p.grad - plain[k]).norm()) for k, p in net.named_parameters()}
  net.zero_grad(set_to_none=True)
  red = data_parallel.GradAllReducer(net)
  assert all(p.grad.data_ptr() == p._mode_grad_sink.data_ptr() for p in net.parameters())
  for rounds in (1, 2):
    red.zero_grad()
    for _ in range(rounds):
      _loss(net, left, right, gt).backward()
    # The plain route itself is only reproducible to `noise` (vendor atomics, amplified by ~60 BatchNorm layers of a random
    # network; measured up to 6 % of a tensor's norm between two identical launches), so the comparison is in the L2 norm per
    # tensor with a 25 % allowance: a missing or doubled contribution is an O(1) relative error.
    for k, p in net.named_parameters():
      ref = plain[k] * rounds
      err = float((p.grad - ref).norm())
      tol = rounds * (4 * noise[k] + 0.25 * float(plain[k].norm()) + 1e-7)
      assert err <= tol, (k, rounds, err, tol)
  red.detach()
  assert not any(hasattr(p, '_mode_grad_sink') for p in net.parameters())


def test_gradient_carriers_give_autograds_sums_bit_for_bit(monkeypatch):
  """HF.GradCarrier: dres1's input, out1 and out2 have two consumers each; the gradient that arrives first is added inside the kernel
  that produces the second (mode_conv3d_bwd_data_split_acc) instead of by autograd.  a + b is b + a in fp32 and (v + 0) + a is a + v:
  every parameter gradient equals the plain route's bit for bit, also in a second backward on the same graph; and the kernels with
  the add in their store really ran (3 per backward)."""
  from mode_hip import functional as HF
  net, left, right, gt = _tiny_net(11)
  calls, calls2d = [], []
  real, real2d = HF.conv3d_bwd_data, HF.conv2d_bwd_data

  def spy(gy, w, in_shape, stride=1, acc=None, **kw):
    calls.append((stride, acc is not None))
    return real(gy, w, in_shape, stride, acc, **kw)

  def spy2d(gy, w, dilation=1, acc=None, **kw):
    calls2d.append(acc is not None)
    return real2d(gy, w, dilation, acc, **kw)

  monkeypatch.setattr(HF, 'conv3d_bwd_data', spy)
  monkeypatch.setattr(HF, 'conv2d_bwd_data', spy2d)
  grads = {}
  for on in (False, True):
    monkeypatch.setattr(HF, 'GRAD_CARRIERS', on)
    net.zero_grad(set_to_none=True)
    del calls[:], calls2d[:]
    torch.manual_seed(0)
    loss = _loss(net, left, right, gt)
    loss.backward(retain_graph=True)
    grads[on] = {k: p.grad.clone() for k, p in net.named_parameters()}
    n_acc = sum(1 for c in calls if c[1])
    assert n_acc == (3 if on else 0), calls
    # the extractor's regular residual blocks with an identity skip, once per pass of the paired extractor
    n2d = sum(1 for c in calls2d if c)
    blocks = [m for m in net.feature_extraction.modules() if hasattr(m, '_residual') and m.downsample is None and not m.input_shared and
              isinstance(m.conv1[0][0], torch.nn.Conv2d)]  # (layer3[0]'s input also goes into the concatenation: three consumers, no carrier)
    print('identity-skip regular blocks: %d, input gradients with the skip added in the kernel: %d' % (len(blocks), n2d))
    assert n2d == (len(blocks) if on else 0) and len(blocks) >= 10, (n2d, len(blocks), len(calls2d))
    if on:
      assert sorted(c[0] for c in calls if c[1]) == [1, 2, 2]  # dres1's first convolution; the stride-2 convolutions of dres3 / dres4
      net.zero_grad(set_to_none=True)
      del calls[:], calls2d[:]
      loss.backward()  # the same graph again: the carriers are empty after the first pass and work the same way
      assert sum(1 for c in calls if c[1]) == 3 and sum(1 for c in calls2d if c) == len(blocks)
      for k, p in net.named_parameters():
        assert torch.equal(p.grad, grads[True][k]), k
  for k in grads[False]:
    assert torch.equal(grads[False][k], grads[True][k]), k


def test_partial_backward_is_refused_not_silently_wrong(monkeypatch):
  """a backward pass in which only ONE of the two consumers of a carried tensor runs (backward(inputs=[subset])) used to park
  that consumer's gradient for good and hand a stale one to a later pass.  Now the pass raises at its end (the parked tensor is
  released), and a full backward on the retained graph afterwards gives exactly the gradients of the carrier-less route."""
  from mode_hip import functional as HF
  net, left, right, gt = _tiny_net(12)
  grads = {}
  for on in (False, True):
    monkeypatch.setattr(HF, 'GRAD_CARRIERS', on)
    net.zero_grad(set_to_none=True)
    torch.manual_seed(0)
    loss = _loss(net, left, right, gt)
    if on:
      # gradients of the classifier heads' parameters only: the hourglass consumers of out1 / out2 / cost0 are cut off
      subset = [p for k, p in net.named_parameters() if k.startswith('classif')]
      with pytest.raises(RuntimeError, match='GradCarrier'):
        loss.backward(inputs=subset, retain_graph=True)
      net.zero_grad(set_to_none=True)
    loss.backward()
    grads[on] = {k: p.grad.clone() for k, p in net.named_parameters()}
  for k in grads[False]:
    assert torch.equal(grads[False][k], grads[True][k]), k


def test_graph_replay_matches_eager():
  """mode_hip.graph_step.GraphedStep: forward + loss + backward captured into one hipGraph and replayed; same loss and
  gradients as the eager step on the same weights, and new inputs are picked up through the static tensors."""
  from mode_hip import data_parallel
  from mode_hip.graph_step import GraphedStep
  net, left, right, gt = _tiny_net(5)
  red = data_parallel.GradAllReducer(net)

  def body():
    red.zero_grad()
    loss = _loss(net, left, right, gt)
    loss.backward()
    return loss

  gs = GraphedStep(body, (left, right, gt), warmup=1)
  # Every replay -- not only the first -- must give the eager step's BITS: the kernels are deterministic (fixed-order split-K, no
  # atomics) and the graph is a launch optimisation only.  Round 4 found the second and later replays wrong: a hipMemsetAsync inside
  # mode_conv1x1_bwd_data became a graph memset node, and on this ROCm stack such a node takes effect on the first launch only
  # (tools/experiments/graph_memset_probe.py); the library fills with kernels now (csrc/common.h fill_words).
  graph_runs = []
  for _ in range(4):
    red.flat.fill_(float('nan'))  # the replay itself must zero and fill the buffer
    l_graph = float(gs.replay())
    graph_runs.append((l_graph, red.flat.clone()))
  l_eager = float(body())
  names = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
  for r, (lg, g) in enumerate(graph_runs):
    assert lg == l_eager, (r, lg, l_eager)
    assert torch.equal(g, red.flat), 'replay %d: %s' % (r, op_trace.param_report(names, red.flat.cpu(), g.cpu()))
  left2 = torch.roll(left, 5, 2)
  gs.load(left2, torch.roll(right, 5, 2), gt)
  l2 = float(gs.replay())
  assert abs(l2 - float(body())) <= 1e-4 * abs(l2) and abs(l2 - l_graph) > 1e-7


def test_live_graph_survives_table_cache_pressure():
  """a captured hipGraph holds raw addresses of the cached device tables (integer sampling tables, adjoints, plans).
  With a graph alive, push far more geometries through every cache than TABLE_CACHE_ENTRIES: the graph's tables must stay (pinned
  at capture time, functional._LRU) and a replay must give the bits it gave before."""
  from mode_hip import functional as HF
  from mode_hip.graph_step import GraphedStep
  torch.manual_seed(3)
  conv = torch.nn.Conv2d(8, 16, 3, stride=2, padding=1, bias=False).to(DEV)
  x = torch.randn(2, 8, 24, 40, device=DEV, requires_grad=True)

  def body():
    x.grad = None
    conv.weight.grad = None
    y = HF.conv2d_tabled(x, conv)
    y.square().sum().backward()
    return y, x.grad, conv.weight.grad

  gs = GraphedStep(body, (x,), warmup=1)
  first = [t.clone() for t in gs.replay()]
  pinned_before = len(HF._conv_tables.pinned) + len(HF._adjoint_cache.pinned)
  assert pinned_before >= 2  # the table and its adjoint were handed out during the capture
  junk = []
  for i in range(HF.TABLE_CACHE_ENTRIES + 8):  # other geometries: new tables, new adjoints, evictions, allocator reuse
    c2 = torch.nn.Conv2d(4, 4, 3, stride=2, padding=1, bias=False).to(DEV)
    xi = torch.randn(1, 4, 8 + 2 * i, 12, device=DEV, requires_grad=True)
    HF.conv2d_tabled(xi, c2).sum().backward()
    junk.append(torch.full((1 << 18,), float('nan'), device=DEV))  # whatever was freed gets overwritten
  assert len(HF._conv_tables.d) <= HF.TABLE_CACHE_ENTRIES and len(HF._adjoint_cache.d) <= HF.TABLE_CACHE_ENTRIES
  del junk
  again = gs.replay()
  for a, b in zip(first, again):
    assert torch.equal(a, b)
  ref = conv(x.detach())
  assert torch.allclose(first[0], ref, rtol=1e-4, atol=1e-4)


def test_regular_extractor_variant(golden, arith):
  """ModeDisparity(conv='Regular') -- the PSMNet SPP extractor -- on the HIP path against the reference's
  golden vectors: same state_dict, train / eval outputs as close to the fp64 network as the reference's own fp32 run."""
  import json
  z = golden('model_regular.npz')
  maxdisp, H, W, B, seed = [int(v) for v in z['cfg']]
  # ill-conditioned fixture (random initialisation): the mean error against fp64 is round-off amplified ~10^3 x and moves with the
  # summation order -- 4.5e-5 ... 1.3e-4 px over six runs of the fp32 MFMA kernels, 2.4e-4 with all 39 regular 3x3 layers of this
  # variant on the split-bf16 path (kernel by kernel at least as close to fp64, tests/test_gpu_split.py); the reference's own fp32
  # run: 2.9e-5.  The north_star's bound is asserted on the well-conditioned fixtures (tests/test_gpu_parity.py).
  mean_floor = DISP_TOL / 5 if arith == 'f32' else DISP_TOL / 3
  manifest = [(k, tuple(s)) for k, s in json.loads(str(z['manifest']))]
  net = models.ModeDisparity(maxdisp, 'Regular').to(DEV)
  assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == manifest
  net.load_state_dict(recipe.recipe_state(manifest, seed))
  left, right = recipe.recipe_images(B, H, W, seed + 1)
  gt = recipe.recipe_disparity(B, H, W, seed + 2, maxdisp)
  left, right, gt = left.to(DEV), right.to(DEV), gt.to(DEV)
  net.train()
  preds = net(left, right)
  e_ref = max(np.abs(z['train/pred%d' % i] - z['truth64/train_pred%d' % i]).max() for i in (1, 2, 3))
  for i, p in enumerate(preds):
    # This variant's 2-D convolutions run in the vendor library, whose solver choice differs from process to process
    # (measured mean error over six runs: 4.5e-5 ... 1.3e-4 px, the reference's own fp32 run: 2.9e-5; max error 0.8 ... 4.0 x
    # E_ref, the largest on a box where MIOpen's find picked other solvers): floor at DISP_TOL/5, max at 8 x E_ref -- a wrong
    # layer is an O(0.1 .. 1) px difference.
    _check_disp('regular train pred%d' % (i + 1), p[:, :, ::4, ::4], z['train/pred%d' % (i + 1)], z['truth64/train_pred%d' % (i + 1)], e_ref,
                mean_floor=mean_floor, max_factor=8.0)
  loss = mode_ref.training_loss(preds, gt, ~torch.isnan(gt))
  assert abs(float(loss.detach()) - float(z['train/loss'])) < 2e-4 * float(z['train/loss'])
  loss.backward()
  grads = dict(net.named_parameters())
  for n, s in zip(z['train/grad_names'], z['train/grad_abs_sum']):
    # (tensors whose true gradient is zero -- e.g. a convolution bias in front of a BatchNorm -- hold round-off only)
    assert abs(float(grads[str(n)].grad.double().abs().sum()) - s) <= 5e-2 * s + 1e-4, str(n)
  sd = net.state_dict()
  for k in z.files:
    if k.startswith('bn/'):
      sd[k[3:]] = torch.from_numpy(z[k]).to(DEV)
  net.load_state_dict(sd)
  net.eval()
  with torch.no_grad():
    pred = net(left, right)
  _check_disp('regular eval pred3', pred[:, :, ::4, ::4], z['eval/pred3'], z['truth64/eval_pred3'],
              np.abs(z['eval/pred3'] - z['truth64/eval_pred3']).max(), mean_floor=mean_floor, max_factor=8.0)


def test_sphere_layers_on_transposed_storage_match_the_nchw_operator(monkeypatch):
  """layer4 of the spherical extractor (16 SphereConv + BatchNorm/ReLU/add/1x1 conv) end to end on plane-transposed storage
  (SphereConv inside transposed_io()) against the same modules on the NCHW operator: outputs, input and parameter
  gradients, BatchNorm state."""
  import models.submodule as sm
  from mode_hip import functional as HF
  monkeypatch.setattr(HF, 'SPHERE_FWD_MIN_WG', 0)  # the small test geometry too
  res = {}
  for chain in (True, False):
    torch.manual_seed(11)
    fe = sm.sphere_feature_extraction(512, 256, 'Cassini').to(DEV).train()  # layer4 at 128 x 64: all window classes
    fe.transposed_chain = chain
    x = torch.randn(2, 3, 512, 256, device=DEV, requires_grad=True)
    if chain:
      convs = [m for m in fe.layer4.modules() if isinstance(m, sm.SphereConv)]
      assert len(convs) == 16 and all(m.supports_transposed_io(2, x.device) for m in convs)
    y = fe(x)
    (y * torch.linspace(-1, 1, y.numel(), device=DEV).view_as(y)).sum().backward()
    res[chain] = (y.detach(), x.grad.clone(), {k: p.grad.clone() for k, p in fe.named_parameters()},
                  {k: v.clone() for k, v in fe.state_dict().items() if 'running' in k})
  a, b = res[True], res[False]
  assert (a[0] - b[0]).abs().max() <= 1e-4 * max(1.0, float(b[0].abs().max()))
  # gradients through ~50 random train-mode BatchNorm layers: round-off of the two summation orders is amplified to ~5e-3
  # (measured); a wrong axis order anywhere would be an O(1) difference
  assert float((a[1] - b[1]).norm()) <= 2e-2 * float(b[1].norm())
  for k in a[2]:
    assert float((a[2][k] - b[2][k]).norm()) <= 2e-2 * float(b[2][k].norm()) + 1e-4, k
  for k in a[3]:
    assert (a[3][k] - b[3][k]).abs().max() <= 1e-5 * max(1.0, float(b[3][k].abs().max())), k


def test_fast_paths_together_match_the_plain_composition(monkeypatch):
  """Every restructuring of the default path switched off at once -- two extractor passes, NCHW spherical operator, cost volume +
  conv3d 64 -> 32, vendor forward / gradients for ALL regular 2-D convolutions -- against the default path, at BASELINE config 1
  size (512 x 256, 64 disparities), batch 2: predictions, loss, gradients, BatchNorm state.  On the well-conditioned recipe state
  of the parity tier (tests/golden/recipe.py), so that the bounds are the parity tier's own -- 1e-3 px on every prediction, 1e-3
  relative L2 on the whole gradient, 5e-2 on every tensor: a subtly wrong fast path does not pass."""
  import recipe
  import models.stage3d as st
  sd = recipe.recipe_state_wc(recipe.load_manifest(), 421)
  left, right = recipe.recipe_images(2, 512, 256, 422, shift=3)
  gt = recipe.recipe_disparity_smooth(2, 512, 256, 423, 64)
  res = {}
  for fast in (True, False):
    net = models.ModeDisparity(64, 'Sphere', 512, 256, 'Cassini').to(DEV)
    net.load_state_dict(sd)
    net.train()
    net.pair_extractor = net.fold_cost_volume = net.feature_extraction.transposed_chain = fast
    if not fast:  # the regular 3x3 layers as the torch modules they are (vendor library)
      own = st.conv3
      monkeypatch.setattr(st, 'conv3', lambda conv, x, *carrier: conv(x) if type(conv) is torch.nn.Conv2d else own(conv, x, *carrier))
    preds = net(left.to(DEV), right.to(DEV))
    g = gt.to(DEV)
    loss = mode_ref.training_loss(preds, g, ~torch.isnan(g))
    loss.backward()
    res[fast] = ([p.detach() for p in preds], float(loss), {k: p.grad.clone() for k, p in net.named_parameters()},
                 {k: v.clone() for k, v in net.state_dict().items() if 'running' in k})
  a, b = res[True], res[False]
  err = max(float((x - y).abs().max()) for x, y in zip(a[0], b[0]))
  num = sum(float((a[2][k].double() - b[2][k].double()).pow(2).sum()) for k in a[2])
  den = sum(float(b[2][k].double().pow(2).sum()) for k in a[2])
  worst = max((float((a[2][k] - b[2][k]).norm()) / (float(b[2][k].norm()) + 1e-12), k) for k in a[2] if float(b[2][k].norm()) > 1e-6 * den**0.5)
  print('fast paths vs plain composition 512x256/64: max |disp diff| %.2e px, loss %.6f vs %.6f, whole gradient rel %.2e, worst tensor %.2e (%s)' %
        (err, a[1], b[1], (num / den)**0.5, worst[0], worst[1]))
  assert err <= 1e-3
  assert abs(a[1] - b[1]) <= 2e-5 * abs(b[1])
  assert (num / den)**0.5 <= 1e-3
  assert worst[0] <= 5e-2, worst
  for k in a[3]:
    assert (a[3][k] - b[3][k]).abs().max() <= 1e-4 * max(1.0, float(b[3][k].abs().max())), k


def test_paired_extractor_pass_equals_two_passes(monkeypatch):
  """ModeDisparity runs the shared extractor once over [left; right] with per-image-set BatchNorm statistics
  (stage3d.bn_groups): same outputs, gradients and BatchNorm state as the reference's two passes."""
  import models.mode_disparity as md
  res = {}
  for paired in (True, False):
    net, left, right, gt = _tiny_net(9)
    net.pair_extractor = paired
    _loss(net, left, right, gt).backward()
    res[paired] = (net(left, right)[2].detach(), {k: p.grad.clone() for k, p in net.named_parameters()},
                   {k: v.clone() for k, v in net.state_dict().items() if 'running' in k or 'num_batches' in k})
  a, b = res[True], res[False]
  # same network, different vendor algorithms at batch 4 vs 2: fp32 round-off, amplified by the random network (the golden
  # tests above hold the paired path to the reference's own error level)
  assert (a[0] - b[0]).abs().max() < 5e-2 and (a[0] - b[0]).abs().mean() < 2e-3
  for k in a[1]:
    assert float((a[1][k] - b[1][k]).norm()) <= 0.25 * float(b[1][k].norm()) + 1e-6, k
  for k in a[2]:
    if 'num_batches' in k:
      assert int(a[2][k]) == int(b[2][k]), k
    else:
      assert (a[2][k] - b[2][k]).abs().max() <= 1e-4 * max(1.0, float(b[2][k].abs().max())), k


# ------------------------------------------------------------------ nn.DataParallel: forward() from one thread per replica
def _replica_pair(seed=13):
  import copy
  torch.manual_seed(seed)
  net = models.ModeDisparity(32, 'Sphere', 128, 64, 'Cassini').to(DEV).train()
  left = torch.randn(2, 3, 128, 64, device=DEV)
  right = torch.roll(left, -3, 3) + 0.01 * torch.randn_like(left)
  return net, copy.deepcopy, left, right


def test_forward_from_two_threads_equals_sequential_runs():
  """The reference's six call sites wrap the module in nn.DataParallel (train_disparity.py:264-265, test_disparity.py:160-161,
  ...): one Python thread per replica calls forward() concurrently.  Two replicas, two threads, two streams of one GPU, train
  mode (so the per-thread BatchNorm grouping of the paired extractor pass is live), many iterations with the threads released
  together: every output and every BatchNorm buffer must equal, bit for bit, the sequential run of the same replica."""
  import threading
  net, clone, left, right = _replica_pair()
  seq = []
  for i in range(2):
    r = clone(net)
    outs = [r(left[i:i + 1] + 0.1 * k, right[i:i + 1] + 0.1 * k) for k in range(4)]
    seq.append(([tuple(o.detach().clone() for o in out) for out in outs], {k: v.clone() for k, v in r.state_dict().items()}))
  torch.cuda.synchronize()
  replicas = [clone(net) for _ in range(2)]
  streams = [torch.cuda.Stream(DEV) for _ in range(2)]
  results, errors = [None, None], []
  gate = threading.Barrier(2)

  def work(i):
    try:
      with torch.cuda.stream(streams[i]):
        outs = []
        for k in range(4):
          gate.wait()
          outs.append(tuple(o.detach() for o in replicas[i](left[i:i + 1] + 0.1 * k, right[i:i + 1] + 0.1 * k)))
        streams[i].synchronize()
        results[i] = outs
    except Exception as e:  # noqa: BLE001
      errors.append(e)
      gate.abort()

  for s_ in streams:
    s_.wait_stream(torch.cuda.current_stream())
  threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
  for t in threads:
    t.start()
  for t in threads:
    t.join()
  assert not errors, errors
  for i in range(2):
    for k in range(4):
      for a, b in zip(results[i][k], seq[i][0][k]):
        assert torch.equal(a, b), (i, k)
    sd = replicas[i].state_dict()
    for key, v in seq[i][1].items():
      assert torch.equal(sd[key], v), (i, key)


def test_under_nn_dataparallel_like_the_reference_call_sites():
  """model = nn.DataParallel(model); model.cuda() -- train_disparity.py:264-265 -- here with both replicas on the one GPU of
  the box (device_ids=[0, 0]): scatter along the batch, one thread per replica, gather.  Per-replica BatchNorm statistics
  (DataParallel semantics), so each half of the batch must equal the module run on that half alone."""
  import copy
  net, clone, left, right = _replica_pair(17)
  want = [clone(net)(left[i:i + 1], right[i:i + 1]) for i in range(2)]
  dp = torch.nn.DataParallel(clone(net), device_ids=[0, 0])
  got = dp(left, right)
  for h in range(3):
    for i in range(2):
      assert torch.equal(got[h][i:i + 1], want[i][h]), (h, i)
  assert [k for k in dp.state_dict()][0].startswith('module.')  # the prefix loadStackHourglassOnly / load_state_dict callers see
  sd = copy.deepcopy(dp.state_dict())
  models.ModeDisparity(32, 'Sphere', 128, 64, 'Cassini').load_state_dict({k[len('module.'):]: v for k, v in sd.items()})


def test_forward_loss_equals_forward_plus_the_references_loss_lines(golden):
  """ModeDisparity.forward_loss (loss + gradient formed next to the heads) against forward() followed by the loss of
  train_disparity.py:151-158 written with torch ops: same predictions (bit for bit), same loss, same gradient of every parameter."""
  import torch.nn.functional as F
  z = golden('model_tiny.npz')
  net, left, right, gt, _ = _setup(z)
  net.train()
  state = {k: v.detach().clone() for k, v in net.state_dict().items()}
  mask = ~torch.isnan(gt)
  o = net(left, right)
  ref = 0.5 * F.smooth_l1_loss(o[0][mask], gt[mask]) + 0.7 * F.smooth_l1_loss(o[1][mask], gt[mask]) + F.smooth_l1_loss(o[2][mask], gt[mask])
  ref.backward()
  want = {k: p.grad.clone() for k, p in net.named_parameters()}
  net.zero_grad()
  with torch.no_grad():
    for k, v in net.state_dict().items():
      v.copy_(state[k])
  loss, preds = net.forward_loss(left, right, gt)
  loss.backward()
  for a, b in zip(o, preds):
    assert torch.equal(a.detach(), b)
  assert abs(float(loss) - float(ref)) <= 2e-6 * abs(float(ref))
  num = sum(float(((p.grad - want[k]).double()**2).sum()) for k, p in net.named_parameters())
  den = sum(float((want[k].double()**2).sum()) for k in want)
  print('forward_loss vs forward + torch loss: whole-network gradient relative L2 %.3e' % (num / den)**0.5)
  assert (num / den)**0.5 <= 1e-5
  net.eval()
  with pytest.raises(RuntimeError, match='training step'):
    net.forward_loss(left, right, gt)


def test_eval_pack_cache_notices_the_librarys_own_training_kernels(golden, monkeypatch):
  """the training BatchNorm kernels write running_mean / running_var through raw pointers.  Eval, then a train-mode forward
  under no_grad (BatchNorm re-estimation: only the running statistics change), then eval again: the second eval must repack -- it equals
  the forward with the cache switched off and differs from the first."""
  from mode_hip import functional as HF
  z = golden('model_tiny.npz')
  net, left, right, _, _ = _setup(z, bn_from_fixture=True)

  def ev(cache):
    monkeypatch.setattr(HF, 'EVAL_PACK_CACHE', cache)
    net.eval()
    with torch.no_grad():
      return net(left, right).clone()

  y0 = ev(True)
  v0 = net.dres0[0][1].running_mean._version
  net.train()
  with torch.no_grad():
    net(left, right)
  assert net.dres0[0][1].running_mean._version > v0 and net.classif1[0][1].running_var._version > 0  # (plain BatchNorm pass and the fused head)
  y1 = ev(True)
  assert torch.equal(y1, ev(False))
  assert not torch.equal(y1, y0)
  # writes torch cannot see need the explicit call
  net.dres2.conv1[0][0].weight.data.mul_(1.05)
  stale = ev(True)
  HF.invalidate_eval_packs(net)
  fresh = ev(True)
  assert torch.equal(fresh, ev(False)) and not torch.equal(fresh, stale)


def test_captured_eval_forward_refuses_to_replay_on_changed_weights(golden):
  """a GraphedStep captured from an eval forward that hit the packed-weight cache replays without pack kernels; it records the
  versions it relied on and raises once a weight has been written (an optimizer step, load_state_dict, an in-place op)."""
  from mode_hip.graph_step import GraphedStep
  z = golden('model_tiny.npz')
  net, left, right, _, _ = _setup(z, bn_from_fixture=True)
  net.eval()

  def fwd():
    with torch.no_grad():
      return net(left, right)

  want = fwd().clone()
  gs = GraphedStep(fwd, (left, right), warmup=1)
  assert gs.frozen and not gs.stale()
  assert torch.equal(gs.replay(), want)
  with torch.no_grad():
    net.dres3.conv2[0].weight.mul_(1.01)
  assert gs.stale()
  with pytest.raises(RuntimeError, match='changed after this graph was captured'):
    gs.replay()
  gs2 = GraphedStep(fwd, (left, right), warmup=1)
  assert torch.equal(gs2.replay(), fwd())


def test_replayed_training_moves_the_versions_of_the_batchnorm_state(golden):
  """a REPLAYED training step updates running_mean / running_var through raw pointers with no Python in between; replay()
  moves their version counters like the eager step does, so a BatchNorm recalibration run as graph replays (weights frozen) is seen by
  the packed-weight cache of the eval forward and by a captured inference graph."""
  from mode_hip.graph_step import GraphedStep
  z = golden('model_tiny.npz')
  net, left, right, _, _ = _setup(z, bn_from_fixture=True)
  net.eval()

  def fwd():
    with torch.no_grad():
      return net(left, right)

  before = fwd().clone()
  ev = GraphedStep(fwd, (left, right), warmup=1)
  assert torch.equal(ev.replay(), before) and not ev.stale()
  net.train()
  for p in net.parameters():
    p.requires_grad_(False)  # recalibration: only the running statistics move

  def recal():
    with torch.no_grad():
      return net(left, right)[2]

  tr = GraphedStep(recal, (left, right), warmup=1)
  bn = net.dres2.conv1[0][1]
  assert any(t is bn.running_mean for t in tr.written) and any(t is bn.running_var for t in tr.written)
  v0, rm0 = bn.running_mean._version, bn.running_mean.clone()
  tr.replay()
  assert bn.running_mean._version > v0 and not torch.equal(bn.running_mean, rm0)
  net.eval()
  assert ev.stale()
  with pytest.raises(RuntimeError, match='changed after this graph was captured'):
    ev.replay()
  after = fwd()  # the eager eval forward repacks with the recalibrated statistics
  assert not torch.equal(after, before)
  assert torch.equal(GraphedStep(fwd, (left, right), warmup=1).replay(), after)


def test_eval_forward_keeps_packed_weights_and_notices_changes(golden, monkeypatch):
  """Inference keeps the packed weights of a layer on its BatchNorm module (functional._eval_wpack) and skips the pack kernels on later
  calls: the kept forward equals the repacking one bit for bit, the second call really reuses (mode_weight_pack_reuse), and an
  in-place change of a weight, of a BatchNorm parameter or a load_state_dict is noticed through the tensors' version counters."""
  from mode_hip import functional as HF
  z = golden('model_tiny.npz')
  net, left, right, _, _ = _setup(z, bn_from_fixture=True)
  net.eval()
  uses = {'reuse': 0, 'pack': 0}
  real = HF._PackReuse

  class Counting(real):

    def __init__(self, on):
      uses['reuse' if on else 'pack'] += 1
      real.__init__(self, on)

  monkeypatch.setattr(HF, '_PackReuse', Counting)

  def forward(cache):
    monkeypatch.setattr(HF, 'EVAL_PACK_CACHE', cache)
    with torch.no_grad():
      return net(left, right).clone()

  y_plain = forward(False)
  uses.update(reuse=0, pack=0)
  y_first = forward(True)
  first = dict(uses)
  y_second = forward(True)
  calls = first['pack'] + first['reuse']  # (a layer applied twice in one forward already reuses on its second call)
  assert first['pack'] > 40, first
  assert uses['pack'] == first['pack'] and uses['reuse'] == first['reuse'] + calls, (first, uses)  # the second pass packed nothing
  assert torch.equal(y_first, y_plain) and torch.equal(y_second, y_plain)
  # in-place changes: a convolution weight, a BatchNorm scale, running statistics
  with torch.no_grad():
    net.dres2.conv1[0][0].weight.mul_(1.02)
    net.feature_extraction.firstconv[0][1].weight.add_(0.01)
    net.dres0[0][1].running_var.mul_(1.1)
  y_changed = forward(True)
  assert bool(torch.isfinite(y_changed).all())
  assert torch.equal(y_changed, forward(False))
  assert not torch.equal(y_changed, y_plain)
  # the state loaded again (load_state_dict copies in place: every version moves)
  net.load_state_dict({k: v.clone() for k, v in net.state_dict().items()})
  assert torch.equal(forward(True), y_changed)
