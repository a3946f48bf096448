"""CPU restatement of the fusion stage (TEST INFRASTRUCTURE ONLY -- imported by tests/ and nothing else).

A functional evaluation of ``ModeFusion.forward`` (models/mode_fusion.py:233-252, 301-313) from a state dict with plain
torch CPU ops, and the training loss of train_fusion.py:82-88, 99-112.  Pinned against the imported reference by
tests/golden/fusion_tiny.npz (tests/golden/make_golden_fusion.py; the reference file needs no stand-ins at all).

The network is piecewise linear up to its BatchNorms and the head: which piece a run is on is decided by the sign of every ReLU
input and the argmax of every pooling window.  ``Decisions`` records those of a run, in call order, or replays given ones (so that a
float64 evaluation can be made on the piece another run -- an fp32 one, the GPU's -- was on; tests/fusion_grad_ref.py)."""
import functools

import torch
import torch.nn.functional as F


class Decisions(object):
  """The ReLU and max-pool calls of one evaluation, in call order.

  Record mode (``replay`` None): relu / pool are F.relu / F.max_pool2d; ``made`` keeps ('relu', x > 0) / ('pool', argmax) per call
  (argmax: the flat index into the H * W plane, as ``return_indices`` gives it), ``pre`` the detached input of each call.
  Replay mode: ``replay`` is such a list; relu is ``x * mask`` and pool a gather by the given indices, whatever x holds, and ``made``
  / ``pre`` still report what this run would have decided on its own."""

  def __init__(self, replay=None):
    self.replay, self.made, self.pre = replay, [], []

  def _given(self, kind, shape):
    i = len(self.made) - 1
    assert self.replay is not None and i < len(self.replay), 'call %d (%s): the replayed run made %d calls' % (i, kind, len(self.replay or ()))
    k, d = self.replay[i]
    assert k == kind and tuple(d.shape) == tuple(shape), 'call %d: %s %s here, %s %s in the replayed run' % (i, kind, tuple(shape), k, tuple(d.shape))
    return d

  def relu(self, x):
    self.pre.append(x.detach())
    self.made.append(('relu', x.detach() > 0))
    if self.replay is None:
      return F.relu(x)
    return x * self._given('relu', x.shape).to(x.dtype)

  def pool(self, x):
    y, idx = F.max_pool2d(x, 2, 2, return_indices=True)
    self.pre.append(x.detach())
    self.made.append(('pool', idx))
    if self.replay is None:
      return y
    given = self._given('pool', idx.shape)
    return x.flatten(2).gather(2, given.flatten(2)).view(given.shape)


class _Free(object):
  """No recording: the calls as they always were."""
  relu = staticmethod(F.relu)

  @staticmethod
  def pool(x):
    return F.max_pool2d(x, 2, 2)


def _conv3(P, key, x):
  return F.conv2d(x, P[key], None, 1, 1)


_sigmoid = torch.sigmoid


def _bn(P, key, x, train):
  return F.batch_norm(x, P[key + '.running_mean'], P[key + '.running_var'], P[key + '.weight'], P[key + '.bias'], train, 0.1, 1e-5)


def _block(P, key, x, train, dec=_Free):
  """BasicBlock: conv1 = Sequential(Sequential(Conv2d, BN), ReLU), conv2 likewise (mode_fusion.py:21-34)."""
  for c in ('conv1', 'conv2'):
    x = dec.relu(_bn(P, '%s.%s.0.1' % (key, c), _conv3(P, '%s.%s.0.0.weight' % (key, c), x), train))
  return x


def _layer(P, key, x, train, pool=False, blocks=1, up=False, head=False, dec=_Free, taps=None):
  i = 0
  if pool:
    x = dec.pool(x)
    i += 1
  for _ in range(blocks):
    x = _block(P, '%s.%d' % (key, i), x, train, dec)
    i += 1
  if up:
    x = F.conv_transpose2d(x, P['%s.%d.weight' % (key, i)], P['%s.%d.bias' % (key, i)], 2)
    if taps is not None:
      taps['%s.%d' % (key, i)] = x  # the ConvTranspose output (its bias gradient is a structural zero in front of a train-mode BatchNorm)
    x = dec.relu(_bn(P, '%s.%d' % (key, i + 1), x, train))
  if head:
    x = _sigmoid(F.conv2d(x, P['%s.%d.weight' % (key, i)], P['%s.%d.bias' % (key, i)]))
  return x


def mode_fusion(P, depthes, confs, rgbs, maxdepth, train, decisions=None, taps=None):
  """decisions: a Decisions to record into / replay from (None: plain F.relu / F.max_pool2d).  taps: a dict that receives the
  outputs of the three ConvTranspose2d layers by their state_dict prefix."""
  dec = decisions if decisions is not None else _Free
  layer = functools.partial(_layer, dec=dec, taps=taps)
  fe = 'feature_extraction.'
  dc = []
  for d, c in zip(depthes, confs):
    dc += [d, c]
  depth_input, rgb_input = torch.cat(dc, 1), torch.cat(rgbs, 1)
  depth1 = layer(P, fe + 'depth_layer1', depth_input, train, blocks=2)
  depth2 = layer(P, fe + 'depth_layer2', depth1, train, pool=True)
  depth3 = layer(P, fe + 'depth_layer3', depth2, train, pool=True)
  depth4 = layer(P, fe + 'depth_layer4', depth3, train, pool=True, up=True)
  rgb1 = layer(P, fe + 'rgb_layer1', rgb_input, train, blocks=2)
  rgb2 = layer(P, fe + 'rgb_layer2', rgb1, train, pool=True)
  rgb3 = layer(P, fe + 'rgb_layer3', rgb2, train, pool=True)
  fusion1 = layer(P, fe + 'fusion_layer1', torch.cat((depth1, rgb1), 1), train, blocks=2)
  fusion2 = layer(P, fe + 'fusion_layer2', torch.cat((depth2, rgb2), 1), train, blocks=2)
  fusion3 = layer(P, fe + 'fusion_layer3', torch.cat((depth3, rgb3), 1), train, blocks=2)
  depth5 = layer(P, fe + 'depth_layer5', torch.cat((fusion3, depth4), 1), train, up=True)
  depth6 = layer(P, fe + 'depth_layer6', torch.cat((fusion2, depth5), 1), train, up=True)
  depth7 = layer(P, fe + 'depth_layer7', torch.cat((fusion1, depth6), 1), train, blocks=2, head=True)
  return depth7 * maxdepth


def baseline(P, depthes, maxdepth, train, decisions=None):
  """feature_extraction_Baseline (mode_fusion.py:37-92): a plain stack of blocks on the six concatenated depth maps, and the head."""
  dec = decisions if decisions is not None else _Free
  fe = 'feature_extraction.'
  x = torch.cat(depthes, 1)
  for i, blocks in enumerate((2, 1, 1, 1, 1, 1), 1):
    x = _layer(P, fe + 'layer%d' % i, x, train, blocks=blocks, dec=dec)
  return _layer(P, fe + 'layer7', x, train, blocks=2, head=True, dec=dec) * maxdepth


def silog_loss(lamda, pred, gt):
  """train_fusion.py:82-88."""
  mask = (gt > 0) * (pred > 0)
  d = torch.log(pred[mask]) - torch.log(gt[mask])
  return torch.mean(torch.square(d)) - lamda * torch.square(torch.mean(d))


def training_loss(output, gt, maxdepth):
  """train_fusion.py:99-112: mask gt <= maxdepth, squeeze the channel, silog with lambda 0.5."""
  mask = gt <= maxdepth
  return silog_loss(0.5, torch.squeeze(output, 1)[mask], gt[mask])
