"""mode_hip.optim.Adam: the update rule of the training step on the library's own kernels (csrc/optim.hip).

Replaces ``optim.Adam(model.parameters(), lr, betas=(0.9, 0.999))`` of the reference (train_disparity.py:293).  One ``step()`` is three
launches whatever the number of parameter tensors and parameter groups -- a deterministic fp64 reduction of the flat gradient (its
norm and the count of its non-finite elements), a one-block launch that decides (skip or step) and derives the per-group constants, and
the update over a chunk table -- and none of them depends on a host value that changes from step to step, so ``step()`` can be captured
into a hipGraph together with the forward and backward pass (graph_step.GraphedStep).

  * All gradients live in ONE flat fp32 buffer, ``p.grad`` being views of it: ``flat_grads=reducer.flat`` adopts the buffer of a
    data_parallel.GradAllReducer, without it the optimizer makes its own.  ``exp_avg`` and ``exp_avg_sq`` are flat buffers of the same layout.
  * ``skip_nonfinite`` (default on): a step whose gradient holds an inf or a NaN writes nothing -- parameters, moments and the step
    counter keep their bits -- and counts in ``skipped_steps``.
  * ``max_grad_norm``: the rule of torch.nn.utils.clip_grad_norm_ on the global norm, applied on the fly; the gradient buffer is NOT scaled.
  * ``grad_norm``, ``found_inf``, ``skipped_steps`` and ``step_count`` are 0-d float64 DEVICE tensors that every step overwrites; ``step()``
    never synchronises and never reads the device.
  * Hyper-parameters are ordinary ``param_groups`` entries.  Outside a capture ``step()`` compares them with what the device holds and
    refreshes it with one non-blocking copy when something changed; between replays of a captured step call ``sync_hyperparameters()``.
  * ``state_dict()`` / ``load_state_dict()`` speak torch.optim.Adam's format in both directions (both read the device: not for the hot path).
The element arithmetic is that of torch's single-tensor path, operation by operation, in fp32."""
import numpy as np
import torch

from . import CONSTANTS, HEADER, _header, check, functional, lib, profiling, ptr, stream_of

CHUNK, STATE_DOUBLES, GROUP_DOUBLES = (CONSTANTS['MODE_ADAM_' + k] for k in 'CHUNK STATE_DOUBLES GROUP_DOUBLES'.split())
S_STEP, S_SKIPPED, S_GRAD_NORM, S_FOUND_INF, S_NONFINITE = (CONSTANTS['MODE_ADAM_' + k] for k in 'STEP SKIPPED GRAD_NORM FOUND_INF NONFINITE'.split())
SEGMENT = np.dtype(_header.structure(HEADER, 'mode_adam_segment'))
CHUNK_RECORD = np.dtype(_header.structure(HEADER, 'mode_adam_chunk'))
_HOST_ROWS = 4  # pinned staging rows of the hyper-parameter refresh (a row is rewritten only after its copy has left it)


def build_tables(numels, groups, addresses=None, chunk=CHUNK):
  """The segment and the chunk table of a flat layout (host code; structured numpy arrays of SEGMENT / CHUNK_RECORD).
  numels[i], groups[i], addresses[i]: size, group index and device address of parameter tensor i; the tensors follow each other
  in the flat layout without padding.  Every chunk lies inside one segment and holds at most `chunk` elements."""
  numels = [int(n) for n in numels]
  if not numels or min(numels) <= 0:
    raise ValueError('build_tables: every parameter tensor needs at least one element')
  if len(groups) != len(numels):
    raise ValueError('build_tables: one group index per tensor')
  seg = np.zeros(len(numels), dtype=SEGMENT)
  seg['numel'] = numels
  seg['first'] = np.cumsum([0] + numels[:-1])
  seg['group'] = groups
  if addresses is not None:
    seg['param'] = addresses
  per_seg = [-(-n // chunk) for n in numels]
  ch = np.zeros(sum(per_seg), dtype=CHUNK_RECORD)
  ch['seg'] = np.repeat(np.arange(len(numels)), per_seg)
  start = np.concatenate([np.arange(k, dtype=np.int64) * chunk for k in per_seg])  # the chunk's first element inside its segment
  ch['off'] = seg['first'][ch['seg']] + start
  ch['count'] = np.minimum(chunk, seg['numel'][ch['seg']] - start)
  return seg, ch


class Adam(torch.optim.Optimizer):

  def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, *, flat_grads=None, skip_nonfinite=True,
               max_grad_norm=None, amsgrad=False, maximize=False):
    if not 0.0 <= lr:
      raise ValueError('Invalid learning rate: %r' % (lr,))
    if not 0.0 <= eps:
      raise ValueError('Invalid epsilon value: %r' % (eps,))
    if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
      raise ValueError('Invalid beta parameters: %r' % (betas,))
    if not 0.0 <= weight_decay:
      raise ValueError('Invalid weight_decay value: %r' % (weight_decay,))
    self._built = False
    # (the keys torch.optim.Adam keeps per group, so that a state_dict changes hands in both directions; only the first four and
    # max_grad_norm are read here)
    defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=None, capturable=False,
                    differentiable=False, fused=None, decoupled_weight_decay=False, max_grad_norm=max_grad_norm)
    torch.optim.Optimizer.__init__(self, params, defaults)
    self._check_groups(self.param_groups)
    self.skip_nonfinite = bool(skip_nonfinite)
    # parameters that take no gradient stay in param_groups (as in torch, whose state_dict numbers them too) and out of the update
    self._params, group_of = [], []
    for gi, g in enumerate(self.param_groups):
      for p in g['params']:
        if p.requires_grad:
          self._params.append(p)
          group_of.append(gi)
    if not self._params:
      raise ValueError('mode_hip.optim.Adam: no parameter requires a gradient')
    dev = self._params[0].device
    for p in self._params:
      if p.dtype != torch.float32:
        raise TypeError('mode_hip.optim.Adam updates fp32 parameters (got %s)' % p.dtype)
      if not p.is_contiguous():
        raise ValueError('mode_hip.optim.Adam needs contiguous parameters')
      if p.device != dev:
        raise ValueError('mode_hip.optim.Adam: all parameters on one device (got %s and %s)' % (dev, p.device))
    if dev.type != 'cuda':
      raise NotImplementedError('Only support cuda tensor!')  # (the refusal of every operator of the package: no CPU path exists)
    self.device = dev
    numels = [p.numel() for p in self._params]
    self.numel = n = sum(numels)
    seg, ch = build_tables(numels, group_of, [p.data_ptr() for p in self._params])
    firsts = [int(v) for v in seg['first']]
    if flat_grads is not None:
      if not (torch.is_tensor(flat_grads) and flat_grads.dtype == torch.float32 and flat_grads.device == dev and flat_grads.dim() == 1 and
              flat_grads.is_contiguous() and flat_grads.numel() == n):
        raise ValueError('flat_grads: one contiguous fp32 buffer of %d elements on %s (GradAllReducer.flat of the same parameters)' % (n, dev))
      for i, (p, first) in enumerate(zip(self._params, firsts)):
        if p.grad is None or p.grad.data_ptr() != flat_grads.data_ptr() + 4 * first or p.grad.numel() != p.numel():
          raise ValueError('flat_grads: the gradient of parameter %d %s is not the view at element %d of the buffer -- the parameter '
                           'order and the .grad views must be those of the GradAllReducer that owns it' % (i, tuple(p.shape), first))
      self.flat = flat_grads
    else:
      self.flat = torch.zeros(n, dtype=torch.float32, device=dev)
    # (parameter, address of its gradient view, its own address, first element, size): what step() verifies and zero_grad() restores
    self._watch = [(p, self.flat.data_ptr() + 4 * first, p.data_ptr(), first, k) for p, first, k in zip(self._params, firsts, numels)]
    self._bind_views()
    self.exp_avg = torch.zeros(n, dtype=torch.float32, device=dev)
    self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=dev)
    self._segments = torch.from_numpy(seg.view(np.uint8).copy()).to(dev)
    self._chunks = torch.from_numpy(ch.view(np.uint8).copy()).to(dev)
    self._n_seg, self._n_chunks, self._n_groups = len(seg), len(ch), len(self.param_groups)
    L = lib()
    self._ws_bytes = int(L.mode_adam_workspace_bytes(n))
    self._workspace = torch.empty(self._ws_bytes // 8, dtype=torch.float64, device=dev)
    self._block = torch.zeros(int(L.mode_adam_block_bytes(self._n_groups)) // 8, dtype=torch.float64, device=dev)
    self._hyper_dev = self._block[STATE_DOUBLES:STATE_DOUBLES + GROUP_DOUBLES * self._n_groups]
    self.step_count = self._block[S_STEP]
    self.skipped_steps = self._block[S_SKIPPED]
    self.grad_norm = self._block[S_GRAD_NORM]
    self.found_inf = self._block[S_FOUND_INF]
    self._host = torch.empty(_HOST_ROWS, GROUP_DOUBLES * self._n_groups, dtype=torch.float64).pin_memory()
    self._host_events, self._host_row = [None] * _HOST_ROWS, 0
    self._held = None  # the hyper-parameters the device block holds
    self.bytes_per_step = 7 * 4 * n + 4 * n  # update: p, m, v read and written + the gradient read; norm pass: the gradient once more
    self._built = True
    self.sync_hyperparameters()

  # ------------------------------------------------------------------ construction helpers
  @staticmethod
  def _check_groups(groups):
    for g in groups:
      if g.get('amsgrad', False):
        raise ValueError('mode_hip.optim.Adam does not implement amsgrad=True')
      if g.get('maximize', False):
        raise ValueError('mode_hip.optim.Adam does not implement maximize=True')
      if g.get('decoupled_weight_decay', False):
        raise ValueError('mode_hip.optim.Adam does not implement decoupled weight decay (AdamW)')

  def add_param_group(self, param_group):
    if getattr(self, '_built', False):
      raise ValueError('mode_hip.optim.Adam: the flat layout is fixed at construction; build a new optimizer (state_dict / load_state_dict carry the state over)')
    return torch.optim.Optimizer.add_param_group(self, param_group)

  def _bind_views(self):
    """p.grad = its view of the flat buffer, wherever it is something else."""
    for p, gaddr, _, first, k in self._watch:
      if p.grad is None or p.grad.data_ptr() != gaddr:
        p.grad = self.flat[first:first + k].view_as(p)
    self._views = [p.grad for p in self._params]  # (kept alive: `p.grad is view` is then the cheap form of the address check)

  def _check_views(self):
    for i, (w, view) in enumerate(zip(self._watch, self._views)):
      p, gaddr, paddr, first, _ = w
      g = p.grad
      if g is not view and (g is None or g.data_ptr() != gaddr):
        raise RuntimeError('mode_hip.optim.Adam: the gradient of parameter %d %s is no longer its view of the flat gradient buffer (element %d) -- '
                           'something replaced it, e.g. a foreign zero_grad(set_to_none=True).  Call zero_grad() of THIS optimizer (or '
                           'GradAllReducer.rebind() of the reducer that owns the buffer) before the backward pass' % (i, tuple(p.shape), first))
      if p.data_ptr() != paddr:
        raise RuntimeError('mode_hip.optim.Adam: parameter %d %s moved to other memory after the optimizer was built; build a new optimizer' %
                           (i, tuple(p.shape)))

  # ------------------------------------------------------------------ hyper-parameters
  def _hyper(self):
    out = []
    for g in self.param_groups:
      mx = g.get('max_grad_norm')
      out.append((float(g['lr']), float(g['betas'][0]), float(g['betas'][1]), float(g['eps']), float(g['weight_decay']), float(mx) if mx else 0.0))
    return out

  def sync_hyperparameters(self):
    """Bring the device block up to date with param_groups (one non-blocking copy, and only when something changed).  step() does this by
    itself outside a capture; call it between the replays of a captured step after changing e.g. the learning rate."""
    want = self._hyper()
    if want == self._held:
      return False
    self._check_groups(self.param_groups)
    r = self._host_row
    ev = self._host_events[r]
    if ev is not None and not ev.query():  # (four refreshes in flight at once: only then is there anything to wait for)
      ev.synchronize()
    row = self._host[r]
    row.copy_(torch.tensor([v for h in want for v in h + (0.0,) * (GROUP_DOUBLES - len(h))], dtype=torch.float64))
    self._hyper_dev.copy_(row, non_blocking=True)
    if row.is_pinned():
      ev = torch.cuda.Event()
      ev.record(torch.cuda.current_stream(self.device))
      self._host_events[r] = ev
    self._host_row = (r + 1) % _HOST_ROWS
    self._held = want
    return True

  # ------------------------------------------------------------------ the step
  def zero_grad(self, set_to_none=True):
    """One fill of the flat buffer; the .grad views stay (and come back if something replaced them) whatever `set_to_none` says --
    torch's default would detach them from the buffer the kernels read."""
    self._bind_views()
    self.flat.zero_()

  def step(self, closure=None):
    loss = None
    if closure is not None:
      with torch.enable_grad():
        loss = closure()
    if not functional._stream_capturing():
      self._check_views()
      self.sync_hyperparameters()
    L = lib()
    st = stream_of(self.flat)
    with profiling.region('adam', self.bytes_per_step, 0, self.device):
      check(L.mode_adam_prepare(ptr(self.flat), self.numel, ptr(self._workspace), self._ws_bytes, ptr(self._block), self._n_groups,
                                int(self.skip_nonfinite), st), 'mode_adam_prepare')
      check(L.mode_adam_update(ptr(self._segments), self._n_seg, ptr(self._chunks), self._n_chunks, ptr(self.flat), ptr(self.exp_avg),
                               ptr(self.exp_avg_sq), ptr(self._block), self._n_groups, st), 'mode_adam_update')
    # the kernels wrote the parameters through raw pointers: torch must see it (version counters; under a GraphedStep capture the
    # parameters are logged, so that every replay moves them too)
    functional._written_by_kernel(*self._params)
    return loss

  # ------------------------------------------------------------------ state interchange (torch.optim.Adam's format)
  def _numbered(self):
    """[(index in torch's numbering, parameter)] over all groups."""
    out, i = [], 0
    for g in self.param_groups:
      for p in g['params']:
        out.append((i, p))
        i += 1
    return out

  def state_dict(self):
    step = float(self.step_count.item())
    where = {id(w[0]): (w[3], w[4]) for w in self._watch}
    state = {}
    if step > 0:  # (like torch: no entries before the first step)
      for i, p in self._numbered():
        if id(p) in where:
          first, k = where[id(p)]
          state[i] = {'step': torch.tensor(step, dtype=torch.float32), 'exp_avg': self.exp_avg[first:first + k].view_as(p).clone(),
                      'exp_avg_sq': self.exp_avg_sq[first:first + k].view_as(p).clone()}
    groups, i = [], 0
    for g in self.param_groups:
      packed = {k: v for k, v in g.items() if k != 'params'}
      packed['params'] = list(range(i, i + len(g['params'])))
      i += len(g['params'])
      groups.append(packed)
    return {'state': state, 'param_groups': groups}

  def load_state_dict(self, state_dict):
    groups, state = state_dict['param_groups'], state_dict['state']
    if len(groups) != len(self.param_groups) or any(len(a['params']) != len(b['params']) for a, b in zip(groups, self.param_groups)):
      raise ValueError('loaded state dict has other parameter groups than this optimizer')
    self._check_groups(groups)
    where = {id(w[0]): (w[3], w[4]) for w in self._watch}
    index_of = [i for g in groups for i in g['params']]  # the saved numbering, in our order
    found, steps, missing = [], [], 0
    for (_, p), i in zip(self._numbered(), index_of):
      if id(p) not in where:
        continue
      st = state.get(i, state.get(str(i)))
      if not st:
        missing += 1
        continue
      if st['exp_avg'].numel() != p.numel() or st['exp_avg_sq'].numel() != p.numel():
        raise ValueError('loaded state of parameter %d has %d elements, the parameter %d' % (i, st['exp_avg'].numel(), p.numel()))
      steps.append(float(st['step']))
      found.append((where[id(p)], st))
    if found and missing:
      raise ValueError('loaded state dict holds the state of %d of %d parameters: one step counter serves them all' % (len(found), len(found) + missing))
    if len(set(steps)) > 1:
      raise ValueError('loaded state dict has different step counts (%s): one step counter serves all parameters of a group' % sorted(set(steps)))
    for g, saved in zip(self.param_groups, groups):
      for k, v in saved.items():
        if k != 'params':
          g[k] = v
    self.exp_avg.zero_()
    self.exp_avg_sq.zero_()
    with torch.no_grad():
      for (first, k), st in found:
        self.exp_avg[first:first + k].copy_(st['exp_avg'].reshape(-1))
        self.exp_avg_sq[first:first + k].copy_(st['exp_avg_sq'].reshape(-1))
      self.step_count.fill_(steps[0] if steps else 0.0)
    self._held = None
    self.sync_hyperparameters()
