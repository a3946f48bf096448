"""Float64 reference of BatchNorm (+ residual add) (+ ReLU), its backward pass and its running statistics, two input generators, and the
case list that tests/test_bn_ref_host.py (CPU tier) and tests/test_gpu_batchnorm_forms.py (GPU tier) share.  Plain numpy / torch on the
CPU, no mode_hip: what is written here is the DEFINITION of the layer (nn.BatchNorm2d/3d in training mode, then `+ add`, then ReLU), not
the kernels of csrc/bn_act.hip.  The host tier holds it to nn.BatchNorm in float64 to 1e-12.

Statistics groups.  With `groups` = G the batch is cut into G runs of B / G consecutive samples and each run is normalised with its own
statistics, as G consecutive calls of the module would do; the affine gradients are summed over the groups and the running statistics
take the groups' updates one after the other, each rounded to float32 like a call of its own.

Yardstick.  `yardstick` evaluates the same composition with torch's CPU float32 batch_norm (and autograd) and returns its max-norm error
against the float64 reference per output tensor: what a careful float32 implementation loses on THESE inputs.  The GPU tier allows a
kernel 4 x that (YARD), under the absolute caps the older BatchNorm tests use (CAPS).

Grid cases (`grid_case`).  y, gout and add are multiples of a power of two `step` inside +-`span`, gamma = 1, and beta is searched so that
no float64 pre-activation (with the add or without) is within 1e-3 of zero: the ReLU mask is then the same in any arithmetic and nothing
has to be left out of a comparison.  The sums a statistics block takes -- (y - K), (y - K)^2, g, g (y - K), g y, K the pivot (the first element of the
group's first sample of the channel) -- are integers below 2^24 in units of step / step^2 over one block's share (`block_of`, the launch
geometry of the source: pick_nsplit / apply_chunks with 256 CUs and 256 threads), so every float32 partial sum is exact in any order,
and below 2^20 for the squares, so that one unit is at least 16 ulps of the partial it belongs to.  Both are asserted by integer
arithmetic.  No aligned piece of four consecutive elements equals the pivot everywhere: losing or repeating any 16-byte piece changes
sum (y - K)^2 by at least one unit.  `exact_forward_sums` / `exact_backward_sums` return the integers.

Random cases (`random_case`).  Seeded normal data as in tests/test_gpu_bn_bwd_gadd.py; asserted: no pre-activation within 1e-5 of zero.
"""
import fractions
import functools

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
NUM_CU, NT = 256, 256  # kNumCU (csrc/common.h) and NT (csrc/bn_act.hip)
YARD = 4.0
CAPS = {'out': lambda ref: 2e-5, 'gy': lambda ref: 5e-5 * max(1.0, ref), 'gadd': lambda ref: 1e-6, 'ggamma': lambda ref: 1e-4 * max(1.0, ref),
        'gbeta': lambda ref: 1e-4 * max(1.0, ref)}

# (shape (B, C, S), groups, step, span): the smallest shapes that reach each regime of the launch geometry
GRID_CASES = [
    ((2, 3, 7), 1, 0.125, 1.0),  # scalar path, under one element per thread
    ((1, 2, 1031), 1, 0.125, 1.0),  # scalar path with remainder
    ((2, 4, 3072), 1, 0.125, 1.0),  # 16-byte tail loop only
    ((2, 3, 4100), 1, 0.125, 1.0),  # unrolled loop once; tail for thread 0 only
    ((1, 3, 16392), 1, 0.125, 1.0),  # 2 blocks per row; unrolled twice; tail in 2 threads
    ((4, 2, 16392), 2, 0.25, 1.0),  # groups x 2 blocks
    ((6, 2, 16392), 3, 0.25, 1.0),
    ((1, 2, 32769), 1, 0.125, 1.0),  # scalar path spread over 4 blocks
    ((1, 2, 2105348), 1, 0.125, 1.0),  # nsplit = 257: second trip of reduce_partials
    ((1, 1, 8396804), 1, 0.125, 1.0),  # nsplit capped at 1024, workspace full to its last float, 1025 apply chunks
]
# what the table claims, checked by the host tier against pick_nsplit / apply_chunks and by the GPU tier against the written workspace slots
GRID_GEOMETRY = {((2, 3, 7), 1): (1, 1), ((1, 2, 1031), 1): (1, 1), ((2, 4, 3072), 1): (1, 1), ((2, 3, 4100), 1): (1, 1),
                 ((1, 3, 16392), 1): (2, 2), ((4, 2, 16392), 2): (2, 2), ((6, 2, 16392), 3): (2, 2), ((1, 2, 32769), 1): (4, 4),
                 ((1, 2, 2105348), 1): (257, 257), ((1, 1, 8396804), 1): (1024, 1025)}
# (tests/test_gpu_kernels.py::test_batchnorm_statistics_do_not_cancel_when_mean_dominates: at mean 100 +- 0.1 the input itself is known to
# 1e-5 relative, the normalised value to 1e-4; that test bounds out and gy by 2e-3 and does not look at the affine gradients -- ggamma
# inherits half an ulp of |mean| x sum g from the float32 saved mean in any implementation, torch's included, so it gets gy's 2e-3 too)
MEAN_DOMINATED_CAPS = dict(CAPS, out=lambda ref: 2e-3, gy=lambda ref: 2e-3 * ref, ggamma=lambda ref: 2e-3 * max(1.0, ref),
                           gbeta=lambda ref: 2e-3 * max(1.0, ref))
RANDOM_SEED = 74


# ------------------------------------------------------------------------------------------------ launch geometry (restated from the source)
def pick_nsplit(rows, S):
  """Statistics blocks per row; rows = channels x groups."""
  n = (64 * NUM_CU + rows - 1) // rows
  n = min(n, max(1, (S // 4) // (8 * NT)))
  return max(1, min(n, 1024))


def apply_chunks(BC, S):
  n = (64 * NUM_CU + BC - 1) // BC
  return max(1, min(n, max(1, (S // 4) // (8 * NT))))


def block_of(S, nsplit):
  """(S,) which statistics block of a row takes each element: NT consecutive 16-byte pieces (rows of whole pieces) or NT consecutive
  elements (other rows) go to one block, dealt out in turn."""
  e = np.arange(S, dtype=np.int64)
  unit = e // 4 if S % 4 == 0 else e
  return (unit // NT) % nsplit


def tail_start_piece(S, nsplit):
  """The first 4-element piece of a row that thread 0 of block 0 leaves to the loop behind the 4 x unrolled one."""
  S4 = S // 4
  st = nsplit * NT
  i = 0
  while i + 3 * st < S4:
    i += 4 * st
  return min(i, S4 - 1)


# ------------------------------------------------------------------------------------------------ the definition, float64
def _grouped(t, groups):
  B = t.shape[0]
  assert B % groups == 0
  return t.reshape((groups, B // groups) + tuple(t.shape[1:]))


def forward(y, gamma, beta, add=None, relu=False, groups=1, eps=EPS):
  """y (B, C, S); returns float64 tensors: out, pre (B, C, S); mean, var (biased), invstd (groups, C)."""
  y, gamma, beta = y.double(), gamma.double(), beta.double()
  yg = _grouped(y, groups)  # (G, Bg, C, S)
  count = yg.shape[1] * yg.shape[3]
  mean = yg.sum((1, 3)) / count
  var = ((yg - mean[:, None, :, None])**2).sum((1, 3)) / count
  invstd = 1.0 / torch.sqrt(var + eps)
  pre = ((yg - mean[:, None, :, None]) * invstd[:, None, :, None] * gamma[None, None, :, None] + beta[None, None, :, None]).reshape(y.shape)
  if add is not None:
    pre = pre + add.double()
  return {'out': torch.relu(pre) if relu else pre, 'pre': pre, 'mean': mean, 'var': var, 'invstd': invstd, 'count': count}


def running_update(fwd, running_mean, running_var, momentum):
  """The float32 running statistics after the groups' updates, applied one after the other with the unbiased variance."""
  rm, rv = running_mean.clone().float(), running_var.clone().float()
  n = fwd['count']
  for g in range(fwd['mean'].shape[0]):
    unbiased = fwd['var'][g] * n / (n - 1) if n > 1 else fwd['var'][g]
    rm = ((1.0 - momentum) * rm.double() + momentum * fwd['mean'][g]).float()
    rv = ((1.0 - momentum) * rv.double() + momentum * unbiased).float()
  return rm, rv


def backward(y, gout, gamma, fwd, relu=False, groups=1):
  """Gradients of sum(out * gout): gy (B, C, S), gadd (the gradient that reaches the residual), ggamma, gbeta (C,), float64."""
  y, gout, gamma = y.double(), gout.double(), gamma.double()
  g = torch.where(fwd['pre'] > 0, gout, torch.zeros_like(gout)) if relu else gout
  yg, gg = _grouped(y, groups), _grouped(g, groups)
  mean, invstd, n = fwd['mean'][:, None, :, None], fwd['invstd'][:, None, :, None], fwd['count']
  xhat = (yg - mean) * invstd
  sg = gg.sum((1, 3))  # (G, C)
  sgx = (gg * xhat).sum((1, 3))
  gy = gamma[None, None, :, None] * invstd * (gg - sg[:, None, :, None] / n - xhat * sgx[:, None, :, None] / n)
  return {'gy': gy.reshape(y.shape), 'gadd': g, 'ggamma': sgx.sum(0), 'gbeta': sg.sum(0)}


def reference(case, relu, with_add, groups):
  fwd = forward(case['y'], case['gamma'], case['beta'], case['add'] if with_add else None, relu, groups)
  out = dict(fwd)
  out.update(backward(case['y'], case['gout'], case['gamma'], fwd, relu, groups))
  return out


def yardstick(case, relu, with_add, groups, ref=None):
  """{tensor: max |torch CPU float32 - float64 reference|} for out, gy, gadd, ggamma, gbeta."""
  ref = ref if ref is not None else reference(case, relu, with_add, groups)
  y = case['y'].clone().requires_grad_(True)
  gamma, beta = case['gamma'].clone().requires_grad_(True), case['beta'].clone().requires_grad_(True)
  add = case['add'].clone().requires_grad_(True) if with_add else None
  parts = [F.batch_norm(p, None, None, gamma, beta, True, 0.1, EPS) for p in y.chunk(groups, 0)]
  o = torch.cat(parts, 0)
  if with_add:
    o = o + add
  if relu:
    o = torch.relu(o)
  o.backward(case['gout'])
  got = {'out': o.detach(), 'gy': y.grad, 'ggamma': gamma.grad, 'gbeta': beta.grad}
  if with_add:
    got['gadd'] = add.grad
  return {k: float((v.double() - ref[k]).abs().max()) for k, v in got.items()}


def eval_forward(y, gamma, beta, running_mean, running_var, add=None, relu=False, eps=EPS):
  """Eval mode: the running statistics in place of the batch's.  float64 (B, C, S)."""
  rm, rv = running_mean.double()[None, :, None], running_var.double()[None, :, None]
  pre = (y.double() - rm) / torch.sqrt(rv + eps) * gamma.double()[None, :, None] + beta.double()[None, :, None]
  if add is not None:
    pre = pre + add.double()
  return torch.relu(pre) if relu else pre


def eval_yardstick(y, gamma, beta, running_mean, running_var, add, relu, ref):
  o = F.batch_norm(y, running_mean, running_var, gamma, beta, False, 0.0, EPS)
  o = o + add if add is not None else o
  o = torch.relu(o) if relu else o
  return float((o.double() - ref).abs().max())


def bound(name, yard, ref_tensor, caps=CAPS):
  """What a kernel's max-norm error against float64 may be: YARD x the yardstick, never above the cap of the older tests."""
  return min(YARD * yard[name], caps[name](float(ref_tensor.abs().max())))


def ulp32(x):
  """float64 array: the spacing of float32 at |x| (x a numpy array or tensor of any float type)."""
  a = np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)
  return np.spacing(a).astype(np.float64)


# ------------------------------------------------------------------------------------------------ generators
def _pivots(yi, groups):
  """yi (B, C, S) integers -> (G, C) the first element of each group's first sample."""
  return _grouped_np(yi, groups)[:, 0, :, 0]


def _grouped_np(a, groups):
  return a.reshape((groups, a.shape[0] // groups) + a.shape[1:])


@functools.lru_cache(maxsize=2)
def grid_case(shape, groups, seed, step, span):
  B, C, S = shape
  n = int(round(span / step))
  assert n * step == span and np.log2(step) == int(np.log2(step))
  rs = np.random.RandomState(seed)
  yi = rs.randint(-n, n + 1, size=shape).astype(np.int64)
  gi = rs.randint(-n, n + 1, size=shape).astype(np.int64)
  ai = rs.randint(-n, n + 1, size=shape).astype(np.int64)
  # no aligned piece of four equals the pivot everywhere: move the second element of such a piece by one step
  S4 = S // 4
  yg = _grouped_np(yi, groups)  # a view
  K = yg[:, 0, :, 0].copy()
  pieces = yg[..., :4 * S4].reshape(yg.shape[:3] + (S4, 4))
  flat = (pieces == K[:, None, :, None, None]).all(-1)
  moved = np.where(K < n, K + 1, K - 1)
  pieces[..., 1] = np.where(flat, np.broadcast_to(moved[:, None, :, None], flat.shape), pieces[..., 1])
  yg[..., :4 * S4] = pieces.reshape(yg.shape[:3] + (4 * S4,))
  assert not (yg[..., :4 * S4].reshape(yg.shape[:3] + (S4, 4)) == K[:, None, :, None, None]).all(-1).any()
  assert (_pivots(yi, groups) == K).all()
  y = torch.from_numpy((yi * step).astype(np.float32))
  gout = torch.from_numpy((gi * step).astype(np.float32))
  add = torch.from_numpy((ai * step).astype(np.float32))
  gamma = torch.ones(C)
  case = {'y': y, 'gout': gout, 'add': add, 'gamma': gamma, 'yi': yi, 'gi': gi, 'K': K, 'step': step, 'span': span, 'n': n,
          'groups': groups, 'shape': shape}
  case['beta'] = _search_beta(case)
  check_grid_case(case)
  return case


def _search_beta(case):
  """Per channel, the first beta = 0.25 + 0.0037 k (float32) that keeps every pre-activation the case can form -- any grid value of y in
  any group, with any grid value of add or without -- at least 1.5e-3 from zero."""
  y, groups = case['y'], case['groups']
  C, n, step = y.shape[1], case['n'], case['step']
  fwd = forward(y, case['gamma'], torch.zeros(C), None, False, groups)
  values = np.arange(-n, n + 1) * step
  addv = np.concatenate([values, [0.0]])
  beta = np.zeros(C, dtype=np.float32)
  for c in range(C):
    base = np.concatenate([((values - float(fwd['mean'][g, c])) * float(fwd['invstd'][g, c]))[:, None] + addv[None, :] for g in range(groups)]).ravel()
    for k in range(4000):
      b = np.float32(0.25 + 0.0037 * k)
      if np.abs(base + np.float64(b)).min() >= 1.5e-3:
        beta[c] = b
        break
    else:
      raise AssertionError('no beta keeps channel %d off the ReLU threshold' % c)
  return torch.from_numpy(beta)


def check_grid_case(case):
  """Every condition the module docstring states, by integer arithmetic (and the threshold condition in float64 on every element)."""
  B, C, S = case['shape']
  groups, n, step = case['groups'], case['n'], case['step']
  yi, gi, K = case['yi'], case['gi'], case['K']
  assert np.array_equal(case['y'].numpy().astype(np.float64), yi * step) and np.abs(yi).max() <= n and np.abs(gi).max() <= n
  assert (case['gamma'] == 1).all()
  for with_add in (False, True):
    pre = forward(case['y'], case['gamma'], case['beta'], case['add'] if with_add else None, False, groups)['pre']
    assert float(pre.abs().min()) >= 1e-3, 'a pre-activation within 1e-3 of the ReLU threshold'
  nsplit = pick_nsplit(C * groups, S)
  blk = block_of(S, nsplit)
  d = np.abs(_grouped_np(yi, groups) - K[:, None, :, None])  # (G, Bg, C, S)
  per_block = lambda a: np.stack([np.bincount(blk, weights=row, minlength=nsplit) for row in a.sum(1).reshape(-1, S).astype(np.float64)])
  assert per_block(d).max() < 2**24 and per_block(d * d).max() < 2**20
  assert per_block(np.abs(_grouped_np(gi, groups))).max() < 2**24
  assert per_block(np.abs(_grouped_np(gi, groups)) * d).max() < 2**24 and per_block(np.abs(_grouped_np(gi * yi, groups))).max() < 2**24
  S4 = S // 4
  assert not (_grouped_np(yi, groups)[..., :4 * S4].reshape((groups, B // groups, C, S4, 4)) == K[:, None, :, None, None]).all(-1).any()


def exact_forward_sums(case):
  """(G, C) integers: sum (y - K) in units of step, sum (y - K)^2 in units of step^2."""
  d = _grouped_np(case['yi'], case['groups']) - case['K'][:, None, :, None]
  return d.sum((1, 3)), (d * d).sum((1, 3))


def exact_statistics(case):
  """(G, C) float64 mean, biased variance and count from the exact integer sums (rational arithmetic, rounded once)."""
  s0, s1 = exact_forward_sums(case)
  G, C = s0.shape
  count = (case['shape'][0] // G) * case['shape'][2]
  step = fractions.Fraction(case['step'])
  mean, var = np.zeros((G, C)), np.zeros((G, C))
  for g in range(G):
    for c in range(C):
      dm = fractions.Fraction(int(s0[g, c]), count)
      mean[g, c] = float((int(case['K'][g, c]) + dm) * step)
      var[g, c] = float((fractions.Fraction(int(s1[g, c]), count) - dm * dm) * step * step)
  return mean, var, count


def exact_backward_sums(case, mask):
  """(G, C) integers: sum g in units of step, sum g y in units of step^2, g = gout where mask (B, C, S, bool array or None: everywhere)."""
  gi = case['gi'] if mask is None else np.where(mask, case['gi'], 0)
  g = _grouped_np(gi, case['groups'])
  return g.sum((1, 3)), (g * _grouped_np(case['yi'], case['groups'])).sum((1, 3))


def _rand(shape, seed, scale=1.0):
  return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32))


@functools.lru_cache(maxsize=4)
def random_case(shape, groups, seed=RANDOM_SEED, mean=1.5, std=2.0, margin=1e-5, clear=False):
  """Seeded normal inputs (as tests/test_gpu_bn_bwd_gadd.py draws them; mean / std: scalars or one value per channel).  Asserted: no
  pre-activation, with the add or without, lies within `margin` of zero.  clear: elements of y that do are moved by a tenth of the
  channel's std, away from the threshold, until none is left (where float32 cannot hold the normalised value to 1e-5 -- a channel whose
  mean dominates -- no seed delivers a margin as wide as the arithmetic's own error)."""
  B, C, S = shape
  m = torch.as_tensor(mean, dtype=torch.float32).expand(C)[None, :, None]
  s = torch.as_tensor(std, dtype=torch.float32).expand(C)[None, :, None]
  y = _rand(shape, seed) * s + m
  g = torch.Generator().manual_seed(7)
  gamma = 1 + 0.2 * torch.randn(C, generator=g)
  beta = 0.3 * torch.randn(C, generator=g)
  case = {'y': y, 'add': _rand(shape, seed + 1), 'gout': _rand(shape, seed + 2), 'gamma': gamma, 'beta': beta, 'groups': groups, 'shape': shape}
  for _ in range(20 if clear else 0):
    near = [forward(y, gamma, beta, case['add'] if with_add else None, False, groups)['pre'] for with_add in (False, True)]
    near = [p.sign() * (p.abs() < 2 * margin) for p in near]
    move = torch.where(near[0] != 0, near[0], near[1])
    if not bool((move != 0).any()):
      break
    y += (move * torch.sign(gamma)[None, :, None] * 0.1 * s).float()
  for with_add in (False, True):
    pre = forward(y, gamma, beta, case['add'] if with_add else None, False, groups)['pre']
    assert int((pre.abs() < margin).sum()) == 0, 'an input element sits on the ReLU threshold: choose another seed'
  return case
