"""torch.autograd wrappers over the C-ABI kernels (host-side glue: shapes, workspaces, autograd; no arithmetic of the path is left
to torch or to a vendor library)."""
import collections
import ctypes
import threading

import torch

from . import (CONSTANTS, LR_STATS, METRICS_COUNT, METRICS_MAX_THRESHOLDS, MVP_MAX_SOURCES, MVP_STATS, MVP_WINS, MVR_MAX_CHANNELS, MVR_RESAMPLE, MVR_SPLAT,
               PHOTOMETRIC_MAX_MAPS, PHOTOMETRIC_STATS,
               BnEpilogue, LrParams, MetricsParams, PhotometricParams, check, lib, profiling, ptr, require_f32c, require_gpu, stream_of)


def _call(entry, *args):
  """Run the C entry `entry` and raise on its error code.  `check` and `lib` are this module's globals, looked up at call time: tests
  replace either to see which entries run."""
  check(getattr(lib(), entry)(*args), entry)


def _stream_capturing():
  """True while the calling thread's current stream is being captured into a hipGraph."""
  return torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing()


class _LRU(object):
  """Bounded cache for the per-geometry device tables (sampling tables of the integer-table convolutions, tile plans, adjoint
  tables, transposed tables): a process that evaluates many resolutions (fisheye / 3D60 / Deep360 in one run) would otherwise pin
  one set per shape for ever -- the adjoint of the 7x7 stem at 1024 x 512 alone is ~100 MB.  Callers hold their own lock.

  Graph safety: a captured hipGraph (mode_hip.graph_step, or any torch.cuda.graph capture) bakes the raw addresses of the tables its
  kernels were launched with into its nodes.  An entry that is handed out WHILE A CAPTURE IS ACTIVE is therefore pinned: it no longer
  counts against maxsize and is never evicted (a later replay would read freed or reused memory and return silently wrong numbers).
  Pins are released only by release_graph_pins(), which callers may use once every graph that used the tables is gone."""
  capturing = staticmethod(_stream_capturing)

  def __init__(self, maxsize):
    self.maxsize = maxsize
    self.d = collections.OrderedDict()
    self.pinned = {}

  def _touch(self, key):
    if key in self.pinned:
      return self.pinned[key]
    value = self.d[key]
    if self.capturing():
      self.pinned[key] = self.d.pop(key)
    else:
      self.d.move_to_end(key)
    return value

  def get(self, key, default=None):
    if key in self.pinned or key in self.d:
      return self._touch(key)
    return default

  def __contains__(self, key):
    return key in self.pinned or key in self.d

  def __getitem__(self, key):
    return self._touch(key)

  def __setitem__(self, key, value):
    if key in self.pinned or self.capturing():
      self.d.pop(key, None)
      self.pinned[key] = value
      return
    self.d[key] = value
    self.d.move_to_end(key)
    while len(self.d) > self.maxsize:
      self.d.popitem(last=False)

  def __len__(self):
    return len(self.d) + len(self.pinned)

  def clear(self):
    """Drop every entry, pinned ones included (for callers that know no graph that used them is left)."""
    self.d.clear()
    self.pinned.clear()

  def release_graph_pins(self):
    """Make the pinned entries evictable again (they re-enter the LRU order as the most recent ones)."""
    for key, value in self.pinned.items():
      self.d[key] = value
    self.pinned.clear()
    while len(self.d) > self.maxsize:
      self.d.popitem(last=False)


TABLE_CACHE_ENTRIES = 24  # per cache; one ModeDisparity geometry uses 1 plan, 2 adjoints, 1 transposed table and 5 integer tables


# ------------------------------------------------------------------------------------ cost volume
def cost_volume_fwd(ref, tgt, d4):
  """(B,C,H,W) x2 -> (B,2C,D4,H,W).  Replaces the loop at models/mode_disparity.py:104-113."""
  require_gpu(ref, tgt)
  ref, tgt = ref.contiguous(), tgt.contiguous()
  require_f32c(ref, tgt)
  if ref.shape != tgt.shape or ref.dim() != 4:
    raise ValueError('cost_volume: feature maps must both be (B,C,H,W), got %s and %s' % (tuple(ref.shape), tuple(tgt.shape)))
  B, C, H, W = ref.shape
  cost = torch.empty((B, 2 * C, d4, H, W), dtype=ref.dtype, device=ref.device)
  nbytes = 4 * (2 * ref.numel() + cost.numel())
  with torch.cuda.device_of(ref), profiling.region('cost_volume_fwd', nbytes, 0, ref.device):
    _call('mode_cost_volume_fwd', ptr(ref), ptr(tgt), ptr(cost), B, C, d4, H, W, stream_of(ref))
  return cost


def cost_volume_bwd(gcost, C):
  require_gpu(gcost)
  gcost = gcost.contiguous()
  require_f32c(gcost)
  B, C2, D4, H, W = gcost.shape
  g_ref = torch.empty((B, C, H, W), dtype=gcost.dtype, device=gcost.device)
  g_tgt = torch.empty_like(g_ref)
  nbytes = 4 * (gcost.numel() + 2 * g_ref.numel())
  with torch.cuda.device_of(gcost), profiling.region('cost_volume_bwd', nbytes, 0, gcost.device):
    _call('mode_cost_volume_bwd', ptr(gcost), ptr(g_ref), ptr(g_tgt), B, C, D4, H, W, stream_of(gcost))
  return g_ref, g_tgt


class CostVolumeFunction(torch.autograd.Function):

  @staticmethod
  def forward(ctx, ref, tgt, d4):
    ctx.C = ref.shape[1]
    return cost_volume_fwd(ref, tgt, d4)

  @staticmethod
  def backward(ctx, gcost):
    g_ref, g_tgt = cost_volume_bwd(gcost, ctx.C)
    return g_ref, g_tgt, None


def cost_volume(ref, tgt, d4):
  return CostVolumeFunction.apply(ref, tgt, d4)


# ------------------------------------------------------------------------------------ sphere conv
# ------------------------------------------------------------------------------------ regular 3x3 Conv2d: own weight gradient
CONV2D_F16 = True  # forward and input gradient of the 3 x 3 layers of a TRAINING step on two fp16 pieces / three MFMAs per product


def _conv2d_f16(f16):
  return bool(f16) and CONV2D_F16 and CONV_ARITH == 'bf16x6'


def _conv2d_route(ci, co, H, W, dilation, which, f16):
  """The kernel family of the stride-1 3 x 3 layer ci -> co on H x W images -- which: 0 forward, 1 input gradient, 2 weight gradient:
  'split' (three bf16 pieces) where CONV_ARITH says so and the split kernel is right at this size (mode_conv2d_split_shape_supported: the
  channel grid and every 32-bit contract; the weight gradient takes any channel counts, an image beyond the offsets -- 2048 x 4096 at up
  to 32 channels is the first -- does not fit), 'split_f16' (two fp16 pieces) when the caller also passes f16, else 'f32'.
  f16 is the one argument in which the sites differ: a training call passes _conv2d_f16(its own flag) (CONV2D_F16), the inference
  wrapper CONV2D_EVAL_F16."""
  if not (CONV_ARITH == 'bf16x6' and lib().mode_conv2d_split_shape_supported(ci, co, H, W, dilation, which) == 1):
    return 'f32'
  return 'split_f16' if f16 else 'split'


def _tag2d(name, ci, co, dilation, h, w):
  """Profiling label of a 3 x 3 layer, e.g. conv2d_fwd[32->32 d1 256x128]."""
  return '%s[%d->%d d%d %dx%d]' % (name, ci, co, dilation, h, w) if profiling.ENABLED else name


def conv2d_bwd_weight(gy, x, dilation=1, into=None):
  """Weight gradient (Co, Ci, 3, 3) of a stride-1 3x3 convolution with padding = dilation (1 or 2): mode_conv2d_bwd_weight.
  `into`: add to this tensor (a gradient sink) instead of returning a new one."""
  require_gpu(gy, x)
  require_f32c(gy, x)
  B, Ci, H, W = x.shape
  Co = gy.shape[1]
  assert tuple(gy.shape) == (B, Co, H, W)
  gw = into if into is not None else torch.empty((Co, Ci, 3, 3), dtype=x.dtype, device=x.device)
  flops = 2 * gy.numel() * Ci * 9
  nbytes = 4 * (gy.numel() + x.numel() + gw.numel())
  with torch.cuda.device_of(x), profiling.region(_tag2d('conv2d_bwd_weight', Ci, Co, dilation, H, W), nbytes, flops, x.device):
    ws = torch.empty(max(lib().mode_conv2d_bwd_weight_workspace_bytes(B, Ci, H, W, Co) // 4, 1), dtype=torch.float32, device=x.device)
    route = _conv2d_route(Ci, Co, H, W, dilation, 2, _conv2d_f16(True))  # (a weight gradient is a training step)
    entry = {'f32': 'mode_conv2d_bwd_weight', 'split': 'mode_conv2d_bwd_weight_split', 'split_f16': 'mode_conv2d_bwd_weight_split_f16'}[route]
    am = (ptr(_tagged_abs_max(gy)), ptr(_tagged_abs_max(x))) if route == 'split_f16' else ()
    _call(entry, ptr(gy), ptr(x), *am, ptr(gw), ptr(ws), B, Ci, H, W, Co, dilation, 1 if into is not None else 0, stream_of(x))
  return gw



CONV2D_OWN_MAX_PIXELS = 1024 * 512  # own forward / input gradient up to this H*W


def _conv2d_own(x, w):
  """Whether forward / input gradient of this layer run on mode_conv2d_fwd / _bwd_data.  Measured at the step's 4 images
  (tools/microbench.py --only conv2d): 90-130 TFLOP/s against the vendor's 80-112 at every shape of the extractor, half
  resolution included, and the fusion network's full-resolution layers (1024 x 512: 32.2 -> 31.9 ms per training step); larger
  images stay on the vendor library (untested territory for the tile choice)."""
  co, ci = int(w.shape[0]), int(w.shape[1])
  # the fp32 kernels take up to 128 channels on either side; wider layers (the fusion network's 256-channel bottleneck) need the split
  # kernels in both directions (forward: reduction ci, input gradient: reduction co -- multiples of 16)
  wide_ok = CONV_ARITH == 'bf16x6' and ci % 16 == 0 and co % 16 == 0 and max(ci, co) <= 512
  return (x.shape[2] * x.shape[3] <= CONV2D_OWN_MAX_PIXELS and ((co <= 128 and ci <= 128) or wide_ok) and
          max(co, ci) * x.shape[2] * x.shape[3] < 2**29)


def conv2d_wgrad_supported(x, w, dilation=1):
  """Whether conv2d_bwd_weight has a kernel that is right at this size: the split kernel inside its 32-bit contracts
  (_conv2d_route, which 2), else the fp32 kernel, which addresses a sample with 32-bit lane offsets
  (csrc/conv2d_f32_wgrad.hip; the entry in conv2d.hip refuses max(Ci, Co) * H * W >= 2^29)."""
  co, ci, H, W = int(w.shape[0]), int(w.shape[1]), int(x.shape[2]), int(x.shape[3])
  return _conv2d_route(ci, co, H, W, dilation, 2, False) != 'f32' or max(co, ci) * H * W < 2**29


def _conv2d_run(which, src, w, dilation, f16=False, w_amax=None, amax_out=None):
  """Forward (which 0: src = x) or input gradient (which 1: src = gy) of the 3 x 3 layer with weight w."""
  name = 'conv2d_bwd_data' if which else 'conv2d_fwd'
  require_gpu(src, w)
  require_f32c(src, w)
  B, _, H, W = src.shape
  Co, Ci = w.shape[:2]
  out = torch.empty((B, Ci if which else Co, H, W), dtype=src.dtype, device=src.device)
  flops = 2 * B * H * W * Ci * Co * 9
  nbytes = 4 * (src.numel() + out.numel() + w.numel())
  with torch.cuda.device_of(src), profiling.region(_tag2d(name, Ci, Co, dilation, H, W), nbytes, flops, src.device):
    wp = torch.empty(lib().mode_conv2d_wpack_bytes(Ci, Co) // 4, dtype=torch.float32, device=src.device)
    route = _conv2d_route(Ci, Co, H, W, dilation, which, _conv2d_f16(f16))
    tail = (ptr(out), ptr(wp), B, Ci, H, W, Co, dilation, stream_of(src))
    if route == 'split_f16':
      aw = _weight_abs_max(w, w_amax)
      if amax_out is not None:
        amax_out.append(aw)
      am = (ptr(_tagged_abs_max(src)), ptr(aw))
      _call('mode_conv2d_bwd_data_split_f16' if which else 'mode_conv2d_fwd_split_f16', ptr(src), ptr(w), *am, *((None,) if which else ()), *tail)
    elif route == 'split' and not which:
      _call('mode_conv2d_fwd_split', ptr(src), ptr(w), None, *tail)  # (None: no folded-BatchNorm epilogue)
    else:
      _call('mode_' + name + ('_split' if route == 'split' else ''), ptr(src), ptr(w), *tail)
  return out


def conv2d_fwd(x, w, dilation=1, f16=False, amax_out=None):
  """f16: the caller is a training step (Conv2d3x3Function with gradients being recorded): the split kernel may use the fp16 arithmetic;
  amax_out: a list that receives the weight's maximum buffer when it did (for the layer's backward)."""
  return _conv2d_run(0, x, w, dilation, f16, amax_out=amax_out)


def conv2d_bwd_data(gy, w, dilation=1, acc=None, f16=True, w_amax=None):
  """acc: a gradient of the same tensor that is already there; the sum is returned (added in the split kernel's store where it runs).
  (A backward pass is a training step: the fp16 arithmetic where CONV2D_F16 says so; w_amax: the weight's maximum from the forward.)"""
  if acc is None:
    return _conv2d_run(1, gy, w, dilation, f16, w_amax=w_amax)
  require_gpu(gy, w, acc)
  acc = acc.contiguous()
  require_f32c(gy, w, acc)
  B, _, H, W = gy.shape
  Co, Ci = w.shape[:2]
  route = _conv2d_route(Ci, Co, H, W, dilation, 1, _conv2d_f16(f16))
  if route == 'f32' or tuple(acc.shape) != (B, Ci, H, W):
    return _conv2d_run(1, gy, w, dilation, f16, w_amax=w_amax).add_(acc)
  gx = torch.empty((B, Ci, H, W), dtype=gy.dtype, device=gy.device)
  with torch.cuda.device_of(gy), profiling.region(_tag2d('conv2d_bwd_data', Ci, Co, dilation, H, W),
                                                  4 * (gy.numel() + 2 * gx.numel() + w.numel()), 2 * B * H * W * Ci * Co * 9, gy.device):
    wp = torch.empty(lib().mode_conv2d_wpack_bytes(Ci, Co) // 4, dtype=torch.float32, device=gy.device)
    if route == 'split_f16':
      _call('mode_conv2d_bwd_data_split_f16', ptr(gy), ptr(w), ptr(_tagged_abs_max(gy)), ptr(_weight_abs_max(w, w_amax)), ptr(acc), ptr(gx), ptr(wp),
            B, Ci, H, W, Co, dilation, stream_of(gy))
    else:
      _call('mode_conv2d_bwd_data_split_acc', ptr(gy), ptr(w), ptr(acc), ptr(gx), ptr(wp), B, Ci, H, W, Co, dilation, stream_of(gy))
  return gx


class Conv2d3x3Function(torch.autograd.Function):
  """y = conv2d(x, w, stride 1, padding = dilation).  Weight gradient always on mode_conv2d_bwd_weight (the vendor's runs as an
  NHWC implicit GEMM between two layout transposes); forward and input gradient on mode_conv2d_fwd / _bwd_data where they are
  faster (_conv2d_own), else on the vendor library's fp32 Winograd."""

  @staticmethod
  def forward(ctx, x, w, dilation, carrier=None, training=False):
    ctx.save_for_backward(x, w)
    ctx.dilation = dilation
    ctx.carrier = carrier  # GradCarrier of x (x has one other consumer: the skip of its residual block), or None
    ctx.own = _conv2d_own(x, w)
    ctx.w_amax = None  # the weight's maximum buffer, when the forward ran on the fp16 arithmetic: the input gradient reads the same weight
    if ctx.own:
      keep = []
      y = conv2d_fwd(x, w.contiguous(), dilation, f16=training, amax_out=keep)  # (training: gradients are being recorded -- set by conv2d_3x3)
      ctx.w_amax = keep[0] if keep else None
      return y
    return torch.nn.functional.conv2d(x, w, None, 1, dilation, dilation)

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, gy):
    x, w = ctx.saved_tensors
    dil = ctx.dilation
    gy = gy.contiguous()
    gx = None
    if ctx.needs_input_grad[0]:
      prev = ctx.carrier.take(ctx) if ctx.carrier is not None else None  # the skip's gradient, when it came first (it always does)
      if ctx.own:
        gx = conv2d_bwd_data(gy, w.contiguous(), dil, acc=prev, w_amax=ctx.w_amax)
      else:
        gx = torch.ops.aten.convolution_backward(gy, x, w, None, [1, 1], [dil, dil], [dil, dil], False, [0, 0], 1, [True, False, False])[0]
        if prev is not None:
          gx = gx.add_(prev)
      if prev is None and ctx.carrier is not None and ctx.carrier.leave(gx, ctx):
        gx = None
    gw = None
    if ctx.needs_input_grad[1]:
      sink = grad_sink(w)
      gw = conv2d_bwd_weight(gy, x.contiguous(), dil, into=sink)
      if sink is not None:
        gw = None
    return gx, gw, None, None, None


def conv2d_3x3(x, w, dilation=1, carrier=None):
  """Callers check conv2d_wgrad_supported(x, w) first (models/stage3d.conv3 does)."""
  if carrier is not None:
    carrier.arm(x.requires_grad and torch.is_grad_enabled())
  return Conv2d3x3Function.apply(x, w, dilation, carrier, torch.is_grad_enabled() and (x.requires_grad or w.requires_grad))


# ------------------------------------------------------------------------------------ cost volume + dres0[0][0], fused
class CostConvAssemble(torch.autograd.Function):
  """out (B,Co,D,H,W) from the partial products R, T (B, 9*Co, H, W) -- see cost_conv() and csrc/cost_conv.hip."""

  @staticmethod
  def forward(ctx, R, T, D):
    require_gpu(R, T)
    require_f32c(R, T)
    B, C9, H, W = R.shape
    Co = C9 // 9
    out = torch.empty((B, Co, D, H, W), dtype=R.dtype, device=R.device)
    nbytes = 4 * (R.numel() + T.numel() + out.numel())
    with torch.cuda.device_of(R), profiling.region('cost_conv_assemble_fwd', nbytes, 0, R.device):
      _call('mode_cost_conv_assemble_fwd', ptr(R), ptr(T), ptr(out), B, Co, D, H, W, stream_of(R))
    ctx.D = D
    return out

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, gout):
    gout = gout.contiguous()
    B, Co, D, H, W = gout.shape
    gR = torch.empty((B, 9 * Co, H, W), dtype=gout.dtype, device=gout.device)
    gT = torch.empty_like(gR)
    nbytes = 4 * (gR.numel() + gT.numel() + gout.numel())
    with torch.cuda.device_of(gout), profiling.region('cost_conv_assemble_bwd', nbytes, 0, gout.device):
      _call('mode_cost_conv_assemble_bwd', ptr(gout), ptr(gR), ptr(gT), B, Co, D, H, W, stream_of(gout))
    return gR, gT, None


def _tap_products(fea, wpart):
  """(B, 9*Co, H, W): channel (kd*3+kw)*Co + o = sum_{c,kh} wpart[o,c,kd,kh,kw] * fea[b,c,h+kh-1,w] (zero padding in h): a
  convolution with a 3 x 1 kernel from C to 9*Co channels -- the gather-and-MAC kernels on an integer table (conv2d_tabled: own
  forward, input gradient and weight gradient; autograd carries the weight gradient back through the permutation)."""
  Co, C = wpart.shape[:2]
  wr = wpart.permute(2, 4, 0, 1, 3).reshape(9 * Co, C, 3, 1)          # rows (kd, kw, o), taps kh
  return Conv2dTabledFunction.apply(fea, wr, (1, 1), (1, 0), (1, 1))


def cost_conv_supported(fea, d4, co):
  """Limits of the two assembly kernels (csrc/cost_conv.hip): the adjoint keeps the D4 gradient rows of one (sample, channel,
  image row) in LDS, the forward the 18 partial-product rows; beyond that the caller builds the volume (mode_cost_volume_fwd)
  and runs the 64 -> 32 convolution on it."""
  B, _, H, W = fea.shape
  return 4 * (4 + d4 * (W + 4)) <= 160 * 1024 and 4 * (9 * (W + 2) + 9 * W) <= 160 * 1024 and B * co * H < 2**31


def cost_conv(ref, tgt, weight, d4):
  """conv3d(cost_volume(ref, tgt, d4), weight, stride 1, padding 1) for a (Co, 2C, 3, 3, 3) weight, without the volume:
  models/mode_disparity.py:104-116.  261 GFLOP per sample of the reference layer become 7 GFLOP of GEMM plus one HBM-bound
  assembly pass; differentiable in ref, tgt and weight (the GEMMs through autograd, the assembly through its adjoint kernel)."""
  C = ref.shape[1]
  assert tuple(weight.shape[1:]) == (2 * C, 3, 3, 3) and ref.shape == tgt.shape
  return CostConvAssemble.apply(_tap_products(ref, weight[:, :C]), _tap_products(tgt, weight[:, C:]), d4)


def _sc_dims(x_shape, w_shape, out_hw, stride, groups):
  B, Ci, H, W = x_shape
  Co, Cig, Kh, Kw = w_shape
  if Ci != Cig * groups:
    raise RuntimeError('Input shape and kernel channels wont match: (%d vs %d).' % (Ci, Cig * groups))
  return [B, Ci, H, W, Co, Kh, Kw, stride[0], stride[1], out_hw[0], out_hw[1], groups]


def _tag2(name, w, x):
  """Profiling label with the layer shape, e.g. sphere_conv_fwd[128->128 256x128]."""
  return '%s[%d->%d %dx%d]' % (name, x.shape[1], w.shape[0], x.shape[2], x.shape[3]) if profiling.ENABLED else name


def _wpack(w, groups):
  Co, Cig, Kh, Kw = w.shape
  n = lib().mode_sphere_conv_wpack_bytes(Cig * groups, Co, Kh, Kw, groups)
  if n == 0:
    check(-1, 'mode_sphere_conv_wpack_bytes')
  return torch.empty(n // 4, dtype=torch.float32, device=w.device)


def _check_pos(pos, x, Kh, Kw):
  if pos.dim() != 4 or pos.shape[1] != 2 * Kh * Kw:
    raise RuntimeError('invalid number of channels of position')
  if pos.shape[2] != x.shape[2] or pos.shape[3] != x.shape[3]:
    raise RuntimeError('invalid spatial size of position, expected height: %d, width: %d, BUT got height: %d, width: %d' %
                       (x.shape[2], x.shape[3], pos.shape[2], pos.shape[3]))


def _per_table(cache, lock, pos, extra, build):
  """build() once per (table, extra, device): the idiom of the four table caches below.  The key uses the table's address, so the
  entry is (value, pos): it keeps `pos` alive.  A value may be None (a table without a plan is remembered as such)."""
  key = (pos.data_ptr(), pos._version, tuple(pos.shape)) + tuple(extra) + (str(pos.device),)
  with lock:
    hit = cache.get(key)
    if hit is None:
      hit = cache[key] = (build(), pos)
    return hit[0]


# The plan records: what sphere_plan and sphere_adjplan return.  The kernels trust them blindly ("The plan contract").
#   tiles    int32 device tensor, 4 words per 64 x 4 tile (origin row, origin column, window base row, window base column with the
#            class above bit 16), listed wrap-around tiles first, then mid-window, then compact (small-window) ones
#   counts   (n_small, n_mid, n_wrap)
#   rest     pixels of the non-small tiles, int32 device tensor (the pixel list of the weight gradient); nrest: their number
#   rec_w, rec_off   record weights (4 floats) and LDS offsets of the compact tiles' taps
#   polar    the polar items of the tall-window (mid and wrap-around) tiles as PolarItems, or None where the planner made none
SpherePlan = collections.namedtuple('SpherePlan', 'tiles counts rest nrest rec_w rec_off polar')
#   items    20 int32 words per item; rec_w, rec_off: 288 records per item; n: the number of items
PolarItems = collections.namedtuple('PolarItems', 'items rec_w rec_off n')
#   tiles    the good tiles, int32 device tensor, 4 words each; ngood: their number
#   rec_off, rec_w     four-source records of the good tiles; rec_off2, rec_w2: the two further sources of the six-source class
#   bad_ids  64-pixel tile ids, in plane-transposed storage, of the tiles left to the gather kernel's list form (None if none); nbad: their number
SphereAdjPlan = collections.namedtuple('SphereAdjPlan', 'tiles ngood rec_off rec_w bad_ids nbad rec_off2 rec_w2')

_plan_cache = _LRU(TABLE_CACHE_ENTRIES)
_plan_lock = threading.Lock()
SPHERE_LAYOUT = 'transposed'  # windowed kernels on plane-transposed copies | 'nchw'
SPHERE_FWD_MIN_WG = 200  # fewer workgroups than this: the windowed forward under-fills the chip, use the general kernel
SPHERE_FWD = 'window'  # 'window' (LDS-window kernels where the table allows) | 'gather'


def transpose_planes(t, out=None):
  """(B, C, H, W) -> (B, C, W, H) contiguous (or the inverse into `out`, whose last two sizes are swapped)."""
  require_gpu(t)
  require_f32c(t)
  B, C, H, W = t.shape
  if out is None:
    out = torch.empty((B, C, W, H), dtype=t.dtype, device=t.device)
  with torch.cuda.device_of(t):
    _call('mode_transpose_planes', ptr(t), ptr(out), B * C, H, W, stream_of(t))
  return out


def sphere_plan(pos, kh, kw):
  """Tile plan of the windowed kernels for the sampling table `pos`: a SpherePlan, or None when the table is not spatially compact
  (the general gather kernels are used then).  Built on the host by mode_sphere_plan_build once per (table, device) and cached,
  like the adjoint table."""
  def build():
    H, W = pos.shape[2:]
    host = pos.detach().to('cpu', torch.float32).contiguous()
    n = lib().mode_sphere_plan_max_tiles(H, W)
    tiles = torch.empty(4 * n, dtype=torch.int32)
    counts = torch.zeros(4, dtype=torch.int32)
    _call('mode_sphere_plan_build', ptr(host), H, W, kh, kw, ptr(tiles), ptr(counts))
    c = [int(v) for v in counts]
    plan = None
    if not c[3]:
      rest = torch.empty(H * W, dtype=torch.int32)
      nrest = torch.zeros(1, dtype=torch.int32)
      _call('mode_sphere_plan_rest_pixels', ptr(tiles), ptr(counts), H, W, ptr(rest), ptr(nrest))
      nrest = int(nrest)
      nrec = max(lib().mode_sphere_plan_records_count(c[0]), 1)
      rec_w = torch.zeros(4 * nrec, dtype=torch.float32)
      rec_off = torch.zeros(nrec, dtype=torch.int32)
      if c[0]:
        _call('mode_sphere_plan_records', ptr(host), ptr(tiles), ptr(counts), H, W, ptr(rec_w), ptr(rec_off))
      polar = None
      npmax = lib().mode_sphere_plan_polar_max_items(ptr(counts))
      if npmax and c[0]:
        pitems = torch.zeros(20 * npmax, dtype=torch.int32)
        prw = torch.zeros(4 * 288 * npmax, dtype=torch.float32)
        pro = torch.zeros(288 * npmax, dtype=torch.int32)
        npol = torch.zeros(1, dtype=torch.int32)
        _call('mode_sphere_plan_polar', ptr(host), ptr(tiles), ptr(counts), H, W, ptr(pitems), ptr(prw), ptr(pro), ptr(npol))
        if int(npol) > 0:
          n = int(npol)
          polar = PolarItems(pitems[:20 * n].contiguous().to(pos.device), prw[:4 * 288 * n].contiguous().to(pos.device),
                             pro[:288 * n].contiguous().to(pos.device), n)
      plan = SpherePlan(tiles.to(pos.device), (c[0], c[1], c[2]), rest[:max(nrest, 1)].contiguous().to(pos.device), nrest,
                        rec_w.to(pos.device), rec_off.to(pos.device), polar)
    return plan
  return _per_table(_plan_cache, _plan_lock, pos, (kh, kw), build)


SPHERE_FWD_F16 = True  # the small-window tiles of a TRAINING forward on two fp16 pieces / three MFMAs per product (bf16x6 only)


SPHERE_BWD_F16 = True  # ... and the windowed input gradient (the adjoint on the same kernel structure)


def _tagged_abs_max(t):
  """The maximum buffer of an ACTIVATION or GRADIENT t: the producer's tag (BatchNorm passes), an earlier call's, or a pass -- whose result
  is left as the tag (known_abs_max drops it when t is written; a tensor that lives inside one step)."""
  am = known_abs_max(t)
  if am is None:
    am = abs_max(t)
    _tag_amax(t, am)
  return am


def _weight_abs_max(w, given=None):
  """The maximum buffer of a WEIGHT: the one the layer's forward computed when the caller kept it (`given`: autograd functions carry it from
  their forward to their backward, where the weight is the same tensor by autograd's own rules), else the entry of the forward pass's
  batched table (weight_maxima: all of a model's weights in one launch at the top of its forward), else a pass.  Never cached on the
  parameter: a write through `.data` moves no version counter, and a stale maximum of a weight that grew is an fp16 overflow -- the
  table lives for ONE forward pass and is computed inside it."""
  if given is not None:
    return given
  table = getattr(_wmax_tls, 'table', None)
  if table is not None:
    hit = table.get(w.data_ptr())
    if hit is not None and hit[1] == w._version and hit[2] == w.numel():
      return hit[0]
  return abs_max(w)


_wmax_tls = threading.local()


class weight_maxima(object):
  """with weight_maxima(module): ...   Inside, the maximum buffers of ALL convolution weights of `module` come from ONE launch
  (mode_abs_max_batch: one workgroup per tensor) issued on entry, instead of a zero fill + a pass per layer -- 63 + 63 launches of ~4.5 us
  per training step of ModeDisparity (0.6 ms of 55).  Only while the fp16 arithmetic is on and gradients are being recorded; the
  table of device pointers is kept on the module (rebuilt when a parameter's storage moved) so that the launch is graph-capturable."""

  def __init__(self, module):
    self.module = module
    self.prev = None

  def __enter__(self):
    self.prev = getattr(_wmax_tls, 'table', None)
    m = self.module
    on = CONV_ARITH == 'bf16x6' and (CONV3D_S1_F16 or SPHERE_FWD_F16 or CONV2D_F16) and torch.is_grad_enabled() and m.training
    ws = [p for p in m.parameters() if p.dim() >= 4 and p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()] if on else []
    if not ws:
      _wmax_tls.table = None
      return self
    key = tuple(p.data_ptr() for p in ws)
    cache = m.__dict__.get('_mode_wmax_cache')
    if cache is None or cache[0] != key:
      dev = ws[0].device
      cache = (key, torch.tensor(key, dtype=torch.int64).to(dev), torch.tensor([p.numel() for p in ws], dtype=torch.int64).to(dev))
      m.__dict__['_mode_wmax_cache'] = cache
    out = torch.empty((len(ws), BN_ABSMAX_FLOATS), dtype=torch.float32, device=ws[0].device)
    with torch.cuda.device_of(out), profiling.region('abs_max_batch', 4 * sum(p.numel() for p in ws), 0, out.device):
      _call('mode_abs_max_batch', ptr(cache[1]), ptr(cache[2]), len(ws), ptr(out), stream_of(out))
    _wmax_tls.table = {p.data_ptr(): (out[i], p._version, p.numel()) for i, p in enumerate(ws)}
    return self

  def __exit__(self, *exc):
    _wmax_tls.table = self.prev
    return False


def _sphere_f16_maxima(x, w, f16):
  """(max |x|, max |w|) buffers for the fp16 arithmetic of the windowed forward, or None when it does not apply."""
  if not (f16 and SPHERE_FWD_F16 and CONV_ARITH == 'bf16x6' and w.shape[1] % 16 == 0):  # (16 input channels per MFMA: the split kernel's layers)
    return None
  return (_tagged_abs_max(x), _weight_abs_max(w))


def _sphere_fwd_route(pos, w, B, groups, stride, same_size, honour_switch, native_t=True):
  """Which kernel runs the spherical forward of weight w on table pos at batch B:
    ('window', plan)    the LDS-window kernels on the tile plan of pos (on plane-transposed copies where SPHERE_LAYOUT says so);
    ('native_t', post)  an ERP-like table: the `_t` operator on the NCHW tensors themselves, with the transposed table post;
    ('gather', None)    the general gather-and-MAC kernel.
  The rule: the geometry of sphere_win_geometry can be planned; a plan of fewer than SPHERE_FWD_MIN_WG workgroups is dropped (one
  workgroup per 64x4 tile, sample and 128-channel slice: below ~one workgroup per CU the general kernel's 64-pixel tiles fill the chip
  better -- measured at B = 1, 256x128: 22.9 vs 20.3 ms for the whole eval forward); an ERP-like table (_sphere_layout) runs on its
  transpose where sphere_t_supported takes that one.
  Where the sites differ:
    honour_switch  whether SPHERE_FWD = 'gather' turns the windowed kernels off: the training operator (sphere_conv_fwd) and
                   sphere_t_supported pass True, the inference wrapper (sphere_conv_bn_eval) passes False -- it never read the switch;
    native_t       False for sphere_t_supported, which asks about the table it was given only."""
  Kh, Kw = w.shape[2:]
  if (honour_switch and SPHERE_FWD != 'window') or not sphere_win_geometry(stride, Kh, Kw, same_size):
    return 'gather', None
  if native_t:
    kind, post = _sphere_layout(pos, Kh, Kw)
    if kind == 'native_t' and sphere_t_supported(post, w, B, groups):
      return 'native_t', post
  plan = sphere_plan(pos, Kh, Kw)
  if plan is not None and sum(plan.counts) * B * groups * (-(-(w.shape[0] // groups) // 128)) < SPHERE_FWD_MIN_WG:
    plan = None
  return ('window', plan) if plan is not None else ('gather', None)


def _sphere_bwd_data_route(pos, kh, kw, stride, same_size, overwrite, have_gyt):
  """Which form runs the input gradient on NCHW tensors (sphere_conv_bwd_data):
    ('scatter', None)    SPHERE_BWD_DATA = 'scatter': the atomic form;
    ('native_t', post)   an ERP-like table: sphere_conv_bwd_data_t on the NCHW tensors themselves, with the transposed table;
    ('copies_t', None)   sphere_conv_bwd_data_t on the plane-transposed copy of the gradient the caller handed in (have_gyt), then a
                         transpose back: only for a caller that lets the result be overwritten;
    ('adjoint', None)    the adjoint gather on the NCHW tensors.
  The two middle answers need SPHERE_BWD_DATA_T.  'copies_t' does not ask for the tap count or the table's kind: whoever hands a
  transposed copy in gets the transposed problem (the adjoint gather has no tap limit of its own)."""
  if SPHERE_BWD_DATA != 'gather':
    return 'scatter', None
  if SPHERE_BWD_DATA_T and sphere_win_geometry(stride, kh, kw, same_size):
    kind, post = _sphere_layout(pos, kh, kw)
    if kind == 'native_t':
      return 'native_t', post
  if SPHERE_BWD_DATA_T and overwrite and have_gyt and sphere_win_geometry(stride, 3, 3, same_size):
    return 'copies_t', None
  return 'adjoint', None


def _sphere_bwd_data_t_route(pos, kh, kw, B, Ci, Co, groups, H, W):
  """Which kernel runs the input gradient on plane-transposed storage (sphere_conv_bwd_data_t): ('window', aplan) the windowed split
  kernel on the adjoint plan of pos plus the gather kernel's list form for the plan's bad tiles, or ('adjoint', None) the adjoint gather
  alone.  The windowed kernel needs the bf16x6 arithmetic, SPHERE_BWD_DATA_SPLIT, channel counts on its grid and an adjoint plan of at
  least SPHERE_BWD_SPLIT_MIN_WG workgroups (one per good tile, sample and 128-channel slice)."""
  if (CONV_ARITH == 'bf16x6' and SPHERE_BWD_DATA_SPLIT and kh * kw == 9 and tuple(pos.shape[2:]) == (H, W) and
      lib().mode_sphere_conv_bwd_data_win_supported(Ci, Co, groups) == 1):
    aplan = sphere_adjplan(pos, kh, kw, f16=SPHERE_BWD_F16)
    if aplan is not None and aplan.ngood * B * groups * (-(-(Ci // groups) // 128)) >= SPHERE_BWD_SPLIT_MIN_WG:
      return 'window', aplan
  return 'adjoint', None


def _sphere_bwd_weight_route(pos, kh, kw, stride, same_size):
  """Which kernel runs the weight gradient on NCHW tensors (sphere_conv_bwd_weight): ('window', plan) the windowed kernels on the
  plan of pos (on plane-transposed copies where SPHERE_LAYOUT says so; a plan that is not usable as a whole runs with its pixel
  list), ('native_t', post) an ERP-like table: sphere_conv_bwd_weight_t on the NCHW tensors, or ('gather', None).  No workgroup
  floor here, and unlike the forward a plan without a compact tile is dropped: nothing to gain."""
  if SPHERE_BWD_WEIGHT != 'window' or not sphere_win_geometry(stride, kh, kw, same_size):
    return 'gather', None
  kind, plan = _sphere_layout(pos, kh, kw)
  if kind == 'native_t':
    return 'native_t', plan
  return ('window', plan) if plan is not None and plan.counts[0] > 0 else ('gather', None)


def sphere_conv_fwd(x, pos, w, out, stride, groups, return_transposed=False, f16=False):
  """Writes `out` (B,Co,Ho,Wo) in place.  Replaces sphere_conv_forward_cuda (sphere_conv_cuda.cpp:129-210).
  return_transposed: return the plane-transposed copy of x the windowed kernel used (None if it did not run) instead of out.
  f16: the caller is a training step (SphereConvFunction with a gradient to compute): the windowed kernel may use the fp16 arithmetic."""
  require_gpu(x, pos, w, out)
  require_f32c(x, pos, w, out)
  _check_pos(pos, x, w.shape[2], w.shape[3])
  dims = _sc_dims(x.shape, w.shape, out.shape[2:], stride, groups)
  flops = 2 * out.numel() * w[0].numel()
  nbytes = 4 * (x.numel() + out.numel() + pos.numel() + w.numel())
  route, plan = _sphere_fwd_route(pos, w, x.shape[0], groups, stride, tuple(out.shape[2:]) == tuple(x.shape[2:]), honour_switch=True)
  if route == 'native_t':
    sphere_conv_fwd_t(x, plan, w, out, groups, f16=f16)
    return None if return_transposed else out
  xt = None
  with torch.cuda.device_of(x), profiling.region(_tag2('sphere_conv_fwd', w, x), nbytes, flops, x.device):
    if route == 'window':
      B, Ci, H, W, Co, Kh, Kw = dims[:7]
      wp = torch.empty(lib().mode_sphere_conv_win_wpack_bytes(Ci, Co, Kh, Kw, groups) // 4, dtype=torch.float32, device=w.device)
      amax = _sphere_f16_maxima(x, w, f16)
      if SPHERE_LAYOUT == 'transposed':
        xt, yt = transpose_planes(x), torch.empty((B, Co, W, H), dtype=x.dtype, device=x.device)
        _sphere_fwd_win(ptr(xt), pos, w, None, ptr(yt), wp, plan, B, Ci, H, W, Co, Kh, Kw, groups, 1, stream_of(x), amax)
        transpose_planes(yt, out)
      else:
        _sphere_fwd_win(ptr(x), pos, w, None, ptr(out), wp, plan, B, Ci, H, W, Co, Kh, Kw, groups, 0, stream_of(x), amax)
    else:
      wp = _wpack(w, groups)
      _call('mode_sphere_conv_fwd', ptr(x), ptr(pos), ptr(w), ptr(out), ptr(wp), *dims, stream_of(x))
  return xt if return_transposed else out


def _sphere_fwd_win(xp, pos, w, e, yp, wp, plan, B, Ci, H, W, Co, Kh, Kw, groups, transposed, stream, amax=None):
  """Windowed spherical forward (optional folded-BatchNorm epilogue `e`): the small-window tiles on the split-bf16 kernel when
  CONV_ARITH says so (the library falls back to the fp32 kernels by itself when the channel count does not fit).
  amax = (max |x|, max |w|) device scalars: the fp16 arithmetic (_sphere_f16_maxima; no epilogue)."""
  tail = (yp, ptr(wp), ptr(plan.tiles)) + tuple(plan.counts) + (B, Ci, H, W, Co, Kh, Kw, groups, transposed, stream)
  if amax is not None and e is None and CONV_ARITH == 'bf16x6':
    _call('mode_sphere_conv_fwd_win_split_f16', xp, ptr(pos), ptr(w), ptr(amax[0]), ptr(amax[1]), *tail)
  elif CONV_ARITH == 'bf16x6':
    _call('mode_sphere_conv_fwd_win_split', xp, ptr(pos), ptr(w), ctypes.byref(e) if e is not None else None, *tail)
  elif e is not None:
    _call('mode_sphere_conv_fwd_win_bn', xp, ptr(pos), ptr(w), ctypes.byref(e), *tail)
  else:
    _call('mode_sphere_conv_fwd_win', xp, ptr(pos), ptr(w), *tail)


_adjoint_cache = _LRU(TABLE_CACHE_ENTRIES)
_adjoint_lock = threading.Lock()
SPHERE_BWD_DATA = 'gather'  # 'gather' (adjoint table) | 'scatter' (atomics)


def sphere_adjoint(pos, kh, kw, stride, out_hw):
  """Device copies (rowptr int32, entries int32 pairs) of the transposed sampling table of `pos`; built on the host by
  mode_sphere_adjoint_build once per (table, stride, output size, device) and cached -- the table is a constant of the
  module (sphere_conv.py:150)."""
  def build():
    H, W = pos.shape[2:]
    host = pos.detach().to('cpu', torch.float32).contiguous()
    nmax = lib().mode_sphere_adjoint_max_entries(kh, kw, out_hw[0], out_hw[1])
    rowptr = torch.empty(kh * kw * H * W + 1, dtype=torch.int32)
    entries = torch.empty(2 * nmax, dtype=torch.int32)
    n = ctypes.c_int64(0)
    _call('mode_sphere_adjoint_build', ptr(host), H, W, kh, kw, stride[0], stride[1], out_hw[0], out_hw[1], ptr(rowptr), ptr(entries),
          ctypes.cast(ctypes.pointer(n), ctypes.c_void_p))
    return rowptr.to(pos.device), entries[:2 * max(n.value, 1)].contiguous().to(pos.device)
  return _per_table(_adjoint_cache, _adjoint_lock, pos, (kh, kw, tuple(stride), tuple(out_hw)), build)


SPHERE_BWD_DATA_T = True  # adjoint gather on plane-transposed storage
_pos_t_cache = _LRU(TABLE_CACHE_ENTRIES)


def _transposed_table(pos):
  """The sampling table of the plane-transposed problem: image (W rows, H columns), row coordinate = the original column
  coordinate and vice versa.  Cached per table like the adjoint."""
  def build():
    K2, H, W = pos.shape[1:]
    p = pos[0].view(K2 // 2, 2, H, W)
    return torch.stack((p[:, 1].transpose(1, 2), p[:, 0].transpose(1, 2)), 1).reshape(1, K2, W, H).contiguous()
  return _per_table(_pos_t_cache, _adjoint_lock, pos, (), build)


def _plan_usable(plan):
  """A plan the windowed forward / weight-gradient kernels can run as a whole: compact tiles exist and the tall-window tiles (if
  any) have polar items.  The question _sphere_layout asks of a table's plan and of its transpose's."""
  return plan is not None and plan.counts[0] > 0 and not (plan.nrest and not (plan.polar is not None and SPHERE_POLAR))


def sphere_win_geometry(stride, kh, kw, same_size):
  """The geometry the windowed kernels and the `_t` operators are written for, stated once: stride (1, 1), 3 x 3 taps and an output
  of the input's size (same_size)."""
  return tuple(stride) == (1, 1) and kh * kw == 9 and bool(same_size)


def _sphere_layout(pos, kh, kw):
  """The kind of the sampling table `pos` -- one answer per table, for all three passes:
    ('copies', plan)    Cassini-like: its own plan is usable as a whole; the windowed kernels run on plane-transposed copies;
    ('native_t', post)  ERP-like: the plan of its transpose post is; the `_t` operators run on the NCHW tensors themselves.  The
                        windowed kernels want the shift-invariant (longitude) axis of the table along the lanes and contiguous in
                        memory.  For the Cassini layout that axis is H, the strided one, hence the copies.  For an ERP table it is W
                        -- already contiguous: an ERP problem on NCHW storage IS the Cassini problem of the transposed table on
                        plane-transposed storage (sphere_conv.py:226-236 builds the Cassini table as exactly that transpose);
    (None, plan)        neither: no 3 x 3 table, SPHERE_LAYOUT 'nchw', or no usable plan either way.  plan is the table's own (or
                        None), for the sites that run a plan that is not usable as a whole.
  SPHERE_LAYOUT and SPHERE_POLAR (_plan_usable) are read at call time."""
  if kh * kw != 9:
    return None, None
  plan = sphere_plan(pos, kh, kw)
  if SPHERE_LAYOUT != 'transposed':
    return None, plan
  if _plan_usable(plan):
    return 'copies', plan
  post = _transposed_table(pos)
  return ('native_t', post) if _plan_usable(sphere_plan(post, kh, kw)) else (None, plan)


def sphere_native_t(pos, kh, kw):
  """sphereType = 'ERP' on the fast path: the transposed table when `pos` itself cannot be planned but its transpose can; else None."""
  kind, post = _sphere_layout(pos, kh, kw)
  return post if kind == 'native_t' else None


def sphere_uses_transposed_copies(pos, kh, kw):
  """Whether the gradients of this table run on plane-transposed COPIES of their operands (Cassini-like tables); ERP-like tables
  (sphere_native_t) and tables without a plan do not."""
  return _sphere_layout(pos, kh, kw)[0] == 'copies'


def sphere_grads_want_transposed_gy(pos, kh, kw, stride, same_size):
  """Whether the caller of the two gradients should hand both one plane-transposed copy of grad_output (sphere_conv_backward_cuda
  asks).  Asked of the table and the geometry only: the copy is also built where SPHERE_BWD_DATA = 'scatter' together with
  SPHERE_BWD_WEIGHT = 'gather' leaves nobody to read it."""
  return sphere_win_geometry(stride, kh, kw, same_size) and sphere_uses_transposed_copies(pos, kh, kw)


def sphere_conv_bwd_data(gy, pos, w, gx, stride, groups, overwrite=False, gy_transposed=None):
  """Accumulates into `gx` (B,Ci,H,W) (caller zero-fills, sphere_conv.py:62); with overwrite=True `gx` may hold anything and
  is overwritten.  gy_transposed: the plane-transposed copy of gy, if the caller has one (the weight gradient needs it too):
  with overwrite=True the gather then runs on the transposed problem, where the 64 lanes of a wave are 64 consecutive rows
  of one column and the source pixels of a tap are runs of consecutive addresses -- on NCHW storage they are one address
  per image row (0.50 vs 0.66 ms per 128->128 layer and 4 images, including the transpose of the result)."""
  require_gpu(gy, pos, w, gx)
  require_f32c(gy, pos, w, gx)
  dims = _sc_dims(gx.shape, w.shape, gy.shape[2:], stride, groups)
  flops = 2 * gy.numel() * w[0].numel()
  nbytes = 4 * (gx.numel() + gy.numel() + pos.numel() + w.numel())
  B, Ci, H, W, Co, Kh, Kw, sH, sW, Ho, Wo, G = dims
  route, post = _sphere_bwd_data_route(pos, Kh, Kw, stride, (Ho, Wo) == (H, W), overwrite,
                                       gy_transposed is not None and tuple(gy_transposed.shape) == (B, Co, Wo, Ho))
  if route == 'native_t':  # the adjoint gather of the transposed problem reads and writes the NCHW tensors directly
    if overwrite:
      return sphere_conv_bwd_data_t(gy, post, w, gx, groups)
    gx += sphere_conv_bwd_data_t(gy, post, w, torch.empty_like(gx), groups)
    return gx
  if route == 'copies_t':  # the operator on the plane-transposed problem (windowed split kernel where the adjoint plan allows), then back
    gxt = sphere_conv_bwd_data_t(gy_transposed, pos, w, torch.empty((B, Ci, W, H), dtype=gx.dtype, device=gx.device), groups)
    with torch.cuda.device_of(gy):
      transpose_planes(gxt, gx)
    return gx
  if route == 'scatter' and overwrite:
    gx.zero_()  # the scatter form adds with atomics
  with torch.cuda.device_of(gy), profiling.region(_tag2('sphere_conv_bwd_data', w, gx), nbytes, flops, gy.device):
    wp = _wpack(w, groups)
    if route == 'scatter':
      _call('mode_sphere_conv_bwd_data', ptr(gy), ptr(pos), ptr(w), ptr(gx), ptr(wp), *dims, stream_of(gy))
    else:
      rowptr, entries = sphere_adjoint(pos, Kh, Kw, stride, gy.shape[2:])
      _call('mode_sphere_conv_bwd_data_adj', ptr(gy), ptr(w), ptr(gx), ptr(wp), ptr(rowptr), ptr(entries), B, Ci, H, W, Co, Kh, Kw, Ho, Wo, G,
            0 if overwrite else 1, stream_of(gy))
  return gx


SPHERE_POLAR = True  # polar kernel for the tall-window tiles (else: pixel list + general kernel)
SPHERE_BWD_WEIGHT_SPLIT = True  # compact-window tiles of the weight gradient on the split-bf16 kernel (CONV_ARITH 'bf16x6' only)


def _bww_win_entry():
  return 'mode_sphere_conv_bwd_weight_win_split' if (CONV_ARITH == 'bf16x6' and SPHERE_BWD_WEIGHT_SPLIT) else 'mode_sphere_conv_bwd_weight_win'


def _bww_f16_maxima(gy, x, gy_src=None, x_src=None):
  """(max |gy|, max |x|) buffers for the fp16 arithmetic of the windowed weight gradient (mode_sphere_conv_bwd_weight_win_split_f16), or
  None when it does not apply.  gy_src / x_src: the tensors the given ones are plane-transposed copies of (same values, maybe tagged)."""
  if not (SPHERE_BWD_F16 and CONV_ARITH == 'bf16x6' and SPHERE_BWD_WEIGHT_SPLIT):
    return None
  def of(t, src):
    am = known_abs_max(t)
    if am is None and src is not None and src is not t:
      am = known_abs_max(src)
    return am if am is not None else _tagged_abs_max(t)
  return (of(gy, gy_src), of(x, x_src))
SPHERE_BWD_WEIGHT = 'window'  # 'window' (where the table allows) | 'gather'


def _sphere_bww_win(gy, x, gyt, xt, pos, gw, plan, use_polar, B, Ci, H, W, Co, groups):
  """The launch of the windowed weight gradient, for both storages: gy, x are the NCHW operands (None on plane-transposed storage),
  gyt, xt their plane-transposed copies (None under SPHERE_LAYOUT 'nchw').  use_polar: the tall-window tiles on the polar kernel
  instead of the pixel list, where the plan has polar items."""
  Kh, Kw = gw.shape[2:]
  tiles, (n0, n1, n2), rest, nrest, rec_w, rec_off, polar = plan
  if polar is not None and use_polar:
    pitems, prw, pro, npol = polar
    nrest = 0
  else:
    pitems = prw = pro = None
    npol = 0
  first = gy if gy is not None else gyt
  n = lib().mode_sphere_conv_bwd_weight_win_workspace_bytes(B, Ci, H, W, Co, Kh, Kw, groups, n0, nrest, npol)
  ws = torch.empty(max(n // 4, 1), dtype=torch.float32, device=first.device)
  entry = _bww_win_entry()
  amax = _bww_f16_maxima(gyt if gyt is not None else gy, xt if xt is not None else x, gy, x)
  if amax is not None:
    entry, amax = entry + '_f16', (ptr(amax[0]), ptr(amax[1]))
  _call(entry, _optr(gy), ptr(pos), _optr(x), *(amax or ()), ptr(gw), ptr(ws), ptr(tiles), n0, n1, n2, ptr(rec_w), ptr(rec_off), ptr(rest), nrest,
        _optr(pitems), _optr(prw), _optr(pro), npol, B, Ci, H, W, Co, Kh, Kw, groups, _optr(gyt), _optr(xt), stream_of(first))


def sphere_conv_bwd_weight(gy, pos, x, gw, stride, groups, x_transposed=None, gy_transposed=None):
  """Accumulates into `gw` (Co,Ci/g,Kh,Kw) (caller zero-fills, sphere_conv.py:63).  x_transposed: the plane-transposed copy
  of x kept from the forward, if any (saves rebuilding it for the windowed kernel); gy_transposed: the same for gy."""
  require_gpu(gy, pos, x, gw)
  require_f32c(gy, pos, x, gw)
  dims = _sc_dims(x.shape, gw.shape, gy.shape[2:], stride, groups)
  B, Ci, H, W, Co, Kh, Kw, sH, sW, Ho, Wo, G = dims
  flops = 2 * gy.numel() * gw[0].numel()
  nbytes = 4 * (x.numel() + gy.numel() + pos.numel() + gw.numel())
  route, plan = _sphere_bwd_weight_route(pos, Kh, Kw, stride, (Ho, Wo) == (H, W))
  if route == 'native_t':
    return sphere_conv_bwd_weight_t(gy, plan, x, gw, groups)
  with torch.cuda.device_of(gy), profiling.region(_tag2('sphere_conv_bwd_weight', gw, x), nbytes, flops, gy.device):
    if route == 'window':
      gyt = xt = None
      if SPHERE_LAYOUT == 'transposed':
        gyt = gy_transposed if gy_transposed is not None and tuple(gy_transposed.shape) == (B, Co, Wo, Ho) else transpose_planes(gy)
        xt = x_transposed if x_transposed is not None and tuple(x_transposed.shape) == (B, Ci, W, H) else transpose_planes(x)
      _sphere_bww_win(gy, x, gyt, xt, pos, gw, plan, SPHERE_POLAR, B, Ci, H, W, Co, G)
    else:
      n = lib().mode_sphere_conv_bwd_weight_workspace_bytes(B, Ci, Co, Kh, Kw, Ho, Wo, G)
      ws = torch.empty(max(n // 4, 1), dtype=torch.float32, device=gy.device)
      _call('mode_sphere_conv_bwd_weight', ptr(gy), ptr(pos), ptr(x), ptr(gw), ptr(ws), *dims, stream_of(gy))
  return gw


# ------------------------------------------------------------------------------------ plane-transposed operator
# A run of stride-1 3x3 spherical layers (layer4 of the extractor: 16 of them, with BatchNorm / ReLU / residual adds in
# between, all of which are indifferent to the order of the two spatial axes) can stay in the (B, C, W, H) storage the
# windowed kernels work on: the three functions below are the operator on that storage, without any transpose.
def sphere_t_supported(pos, w, B, groups):
  """True when the windowed forward would run for this table / weight / batch (else callers use the NCHW operator)."""
  if SPHERE_LAYOUT != 'transposed' or SPHERE_BWD_WEIGHT != 'window' or SPHERE_BWD_DATA != 'gather':
    return False
  route, plan = _sphere_fwd_route(pos, w, B, groups, (1, 1), True, honour_switch=True, native_t=False)
  return route == 'window' and _plan_usable(plan)


def sphere_conv_fwd_t(xt, pos, w, yt, groups, f16=False, amax_out=None):
  """yt (B,Co,W,H) = spherical convolution of xt (B,Ci,W,H), both plane-transposed; stride 1, 3x3 taps.
  amax_out: a list that receives the (max |x|, max |w|) buffers when the fp16 arithmetic ran (for the layer's backward)."""
  require_gpu(xt, pos, w, yt)
  require_f32c(xt, pos, w, yt)
  B, Ci, W, H = xt.shape
  Co, _, Kh, Kw = w.shape
  assert tuple(pos.shape[2:]) == (H, W) and tuple(yt.shape) == (B, Co, W, H)
  plan = sphere_plan(pos, Kh, Kw)
  flops = 2 * yt.numel() * w[0].numel()
  nbytes = 4 * (xt.numel() + yt.numel() + pos.numel() + w.numel())
  with torch.cuda.device_of(xt), profiling.region('sphere_conv_fwd[%d->%d %dx%d]' % (Ci, Co, H, W), nbytes, flops, xt.device):
    wp = torch.empty(lib().mode_sphere_conv_win_wpack_bytes(Ci, Co, Kh, Kw, groups) // 4, dtype=torch.float32, device=w.device)
    amax = _sphere_f16_maxima(xt, w, f16)
    if amax is not None and amax_out is not None:
      amax_out.append(amax)
    _sphere_fwd_win(ptr(xt), pos, w, None, ptr(yt), wp, plan, B, Ci, H, W, Co, Kh, Kw, groups, 1, stream_of(xt), amax)
  return yt


_adjplan_cache = _LRU(TABLE_CACHE_ENTRIES)
SPHERE_BWD_DATA_SPLIT = True  # windowed adjoint on the split-bf16 kernel where the plan allows (CONV_ARITH 'bf16x6' only)
SPHERE_BWD_SPLIT_MIN_WG = 200  # fewer 64 x 4 tiles x samples than this: the 64-pixel tiles of the gather kernel fill the chip better


def sphere_adjplan(pos, kh, kw, f16=None):
  """Adjoint-window plan of the sampling table `pos` (H, W) for the windowed input-gradient kernel, or None when no tile qualifies
  (or H is not a multiple of 64: the left-over tiles are handed to the gather kernel as whole 64-pixel runs of one stored row).
  A SphereAdjPlan.  Built on the host by mode_sphere_adjplan_build once per (table, device), cached.
  f16: the plan of the two-piece fp16 form (None: what SPHERE_BWD_F16 says) -- tiles with an adjoint list heavier than the fp16 headroom
  (2 - 2^-10: the scaled operand would pass 65504) are bad tiles there; the three-piece bf16 form keeps them."""
  def build():
    H, W = pos.shape[2:]
    plan = full = None
    if kh * kw == 9 and H % 64 == 0 and W % 4 == 0:
      host = pos.detach().to('cpu', torch.float32).contiguous()
      n = lib().mode_sphere_plan_max_tiles(H, W)
      good = torch.zeros(4 * n, dtype=torch.int32)
      bad = torch.zeros(2 * n, dtype=torch.int32)
      counts = torch.zeros(2, dtype=torch.int32)
      rec_off = torch.zeros(n * 9 * 256 * 4, dtype=torch.int32)
      rec_w = torch.zeros(n * 9 * 256 * 4, dtype=torch.float32)
      rec_off2 = torch.zeros(n * 9 * 256 * 2, dtype=torch.int32)
      rec_w2 = torch.zeros(n * 9 * 256 * 2, dtype=torch.float32)
      _call('mode_sphere_adjplan_build', ptr(host), H, W, kh, kw, ptr(good), ptr(bad), ptr(counts), ptr(rec_off), ptr(rec_w), ptr(rec_off2),
            ptr(rec_w2))
      ng, nb = int(counts[0]), int(counts[1])
      nh = 0  # the heavy tiles: entries behind the good ones, bit 17 set (bad tiles of the fp16 form)
      while ng + nh < n and (int(good[4 * (ng + nh) + 3]) >> 17) & 1:
        nh += 1
      dev = pos.device

      def make(ng, b2):
        # a bad tile (h0, w0) = the 64-pixel runs h0 .. h0 + 63 of the stored rows w0 .. w0 + 3 of the (W, H) planes
        nb = b2.shape[0]
        ids = ((b2[:, 1:2] + torch.arange(4).view(1, 4)) * H + b2[:, 0:1]) // 64 if nb else torch.zeros((0, 4), dtype=torch.int64)
        ids = ids.reshape(-1).sort().values.to(torch.int32)
        tiles = good[:4 * ng].clone()
        tiles.view(-1, 4)[:, 3] &= ~(1 << 17)
        return SphereAdjPlan(tiles.contiguous().to(dev), ng, rec_off[:ng * 9 * 256 * 4].contiguous().to(dev),
                             rec_w[:ng * 9 * 256 * 4].contiguous().to(dev), ids.contiguous().to(dev) if nb else None, int(ids.numel()),
                             rec_off2[:ng * 9 * 256 * 2].contiguous().to(dev), rec_w2[:ng * 9 * 256 * 2].contiguous().to(dev))
      b2 = bad[:2 * nb].view(nb, 2).to(torch.int64)
      if ng > 0:
        plan = make(ng, b2)
      full = plan
      if nh > 0:
        heavy = {(int(h0), int(w0)) for h0, w0 in good[4 * ng:4 * (ng + nh)].view(nh, 4)[:, :2].tolist()}
        keep = [i for i in range(nb) if (int(b2[i, 0]), int(b2[i, 1])) not in heavy]
        full = make(ng + nh, b2[keep].reshape(-1, 2))
    return plan, full
  plans = _per_table(_adjplan_cache, _plan_lock, pos, (kh, kw), build)
  return plans[0 if (SPHERE_BWD_F16 if f16 is None else f16) else 1]


def sphere_conv_bwd_data_t(gyt, pos, w, gxt, groups, w_amax=None):
  """gxt (B,Ci,W,H) = input gradient for gyt (B,Co,W,H), both plane-transposed (written, not added to)."""
  require_gpu(gyt, pos, w, gxt)
  require_f32c(gyt, pos, w, gxt)
  B, Co, W, H = gyt.shape
  Ci, Kh, Kw = gxt.shape[1], w.shape[2], w.shape[3]
  flops = 2 * gyt.numel() * w[0].numel()
  nbytes = 4 * (gxt.numel() + gyt.numel() + pos.numel() + w.numel())
  rowptr, entries = sphere_adjoint(_transposed_table(pos), Kh, Kw, (1, 1), (W, H))
  route, aplan = _sphere_bwd_data_t_route(pos, Kh, Kw, B, Ci, Co, groups, H, W)
  with torch.cuda.device_of(gyt), profiling.region('sphere_conv_bwd_data[%d->%d %dx%d]' % (Ci, Co, H, W), nbytes, flops, gyt.device):
    wp = _wpack(w, groups)
    if route == 'window':
      tiles, ng, rec_off, rec_w, bad_ids, nbad, rec_off2, rec_w2 = aplan
      wps = torch.empty(lib().mode_sphere_conv_bwd_data_win_wpack_bytes(Ci, Co, Kh, Kw, groups) // 4, dtype=torch.float32, device=w.device)
      tail = (ptr(gxt), ptr(wps), ptr(tiles), ng, ptr(rec_off), ptr(rec_w), ptr(rec_off2), ptr(rec_w2), B, Ci, H, W, Co, Kh, Kw, groups, 1, stream_of(gyt))
      if SPHERE_BWD_F16:  # (a backward pass is a training step: the two-piece fp16 arithmetic)
        _call('mode_sphere_conv_bwd_data_win_split_f16', ptr(gyt), ptr(w), ptr(_tagged_abs_max(gyt)), ptr(_weight_abs_max(w, w_amax)), *tail)
      else:
        _call('mode_sphere_conv_bwd_data_win_split', ptr(gyt), ptr(w), *tail)
      if nbad:  # the tiles next to the poles and the few columns with more than four sources per tap: gather kernel on a tile list
        _call('mode_sphere_conv_bwd_data_adj_list', ptr(gyt), ptr(w), ptr(gxt), ptr(wp), ptr(rowptr), ptr(entries), B, Ci, W, H, Co, Kh, Kw, W, H,
              groups, 0, ptr(bad_ids), nbad, stream_of(gyt))
    else:
      _call('mode_sphere_conv_bwd_data_adj', ptr(gyt), ptr(w), ptr(gxt), ptr(wp), ptr(rowptr), ptr(entries), B, Ci, W, H, Co, Kh, Kw, W, H, groups, 0,
            stream_of(gyt))
  return gxt


def sphere_conv_bwd_weight_t(gyt, pos, xt, gw, groups):
  """Adds the weight gradient for plane-transposed gyt (B,Co,W,H) and xt (B,Ci,W,H) to gw."""
  require_gpu(gyt, pos, xt, gw)
  require_f32c(gyt, pos, xt, gw)
  B, Co, W, H = gyt.shape
  Ci, Kh, Kw = xt.shape[1], gw.shape[2], gw.shape[3]
  plan = sphere_plan(pos, Kh, Kw)
  if plan.nrest and plan.polar is None:
    raise RuntimeError('sphere_conv_bwd_weight_t: the table needs the pixel-list fallback, which reads NCHW tensors')
  flops = 2 * gyt.numel() * gw[0].numel()
  nbytes = 4 * (xt.numel() + gyt.numel() + pos.numel() + gw.numel())
  with torch.cuda.device_of(gyt), profiling.region('sphere_conv_bwd_weight[%d->%d %dx%d]' % (Ci, Co, H, W), nbytes, flops, gyt.device):
    _sphere_bww_win(None, None, gyt, xt, pos, gw, plan, True, B, Ci, H, W, Co, groups)  # (polar items whatever SPHERE_POLAR says: no pixel list here)
  return gw


# ------------------------------------------------------------------------------------ the stride-2 3x3 layer (layer2[0].conv1)
def conv2d_3x3_s2_supported(x, conv):
  """Conv2d(k3, stride 2, padding 1) on even-sized planes, within the limits of the stride-1 kernels its gradients run on."""
  return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and conv.kernel_size == (3, 3) and conv.stride == (2, 2) and
          conv.padding == (1, 1) and conv.dilation == (1, 1) and conv.groups == 1 and conv.bias is None and conv.padding_mode == 'zeros' and
          x.shape[2] % 2 == 0 and x.shape[3] % 4 == 0 and _conv2d_own(x, conv.weight) and conv2d_wgrad_supported(x, conv.weight))


class Conv2d3x3S2Function(torch.autograd.Function):
  """Forward on the integer-table gather kernel; both gradients as stride-1 gradients of the zero-inserted output gradient, on the
  MFMA kernels of the stride-1 layers (csrc/conv2d_f32_fwd.hip, conv2d_f32_wgrad.hip; or their split twins)."""

  @staticmethod
  def forward(ctx, x, w):
    x, w = x.contiguous(), w.contiguous()
    B, Ci, H, W = x.shape
    y = torch.empty((B, w.shape[0], H // 2, W // 2), dtype=x.dtype, device=x.device)
    sphere_conv_fwd(x, conv2d_table(H, W, 3, 3, (2, 2), (1, 1), (1, 1), x.device), w, y, (2, 2), 1)
    ctx.save_for_backward(x, w)
    return y

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, gy):
    x, w = ctx.saved_tensors
    gy = gy.contiguous()
    B, Co, Ho, Wo = gy.shape
    up = torch.empty((B, Co, 2 * Ho, 2 * Wo), dtype=gy.dtype, device=gy.device)
    with torch.cuda.device_of(gy):
      _call('mode_zero_insert2', ptr(gy), ptr(up), B * Co, Ho, Wo, stream_of(gy))
    gx = conv2d_bwd_data(up, w, 1) if ctx.needs_input_grad[0] else None
    gw = None
    if ctx.needs_input_grad[1]:
      sink = grad_sink(w)
      gw = conv2d_bwd_weight(up, x, 1, into=sink)
      if sink is not None:
        gw = None
    return gx, gw


def conv2d_3x3_s2(x, conv):
  return Conv2d3x3S2Function.apply(x, conv.weight)


# ------------------------------------------------------------------------------------ 1x1 Conv2d (stride 1 | 2): plain MFMA GEMMs
def conv1x1_supported(x, conv):
  """The extractor's 1x1 layers (downsample branches, lastconv[0], lastconv[4]) on csrc/conv1x1.hip; the weight gradient loads
  16-byte row pieces, hence the divisibility conditions (other shapes run on the integer-table kernels)."""
  if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and conv.kernel_size == (1, 1) and conv.groups == 1 and
          conv.bias is None and conv.padding == (0, 0) and conv.stride in ((1, 1), (2, 2))):
    return False
  H, W = x.shape[2:]
  s = conv.stride[0]
  return ((W - 1) // s + 1) % 4 == 0 and (s == 1 or W % 8 == 0) and max(conv.in_channels, conv.out_channels) * H * W < 2**31


def _tag1(name, ci, co, s, h, w):
  return '%s[%d->%d s%d %dx%d]' % (name, ci, co, s, h, w) if profiling.ENABLED else name


def conv1x1_fwd(x, w, stride=1, bn=None, add=None, relu=False):
  """y = conv2d(x, w (Co, Ci, 1, 1), stride); with bn: relu?(eval-mode bn(y) [+ add]) in the same launch."""
  require_gpu(x, w)
  x, w = x.contiguous(), w.detach().contiguous() if bn is not None else w.contiguous()
  require_f32c(x, w)
  B, Ci, H, W = x.shape
  Co = w.shape[0]
  y = torch.empty((B, Co, (H - 1) // stride + 1, (W - 1) // stride + 1), dtype=x.dtype, device=x.device)
  flops = 2 * y.numel() * Ci
  with torch.cuda.device_of(x), profiling.region(_tag1('conv1x1_fwd', Ci, Co, stride, H, W), 4 * (x.numel() // stride**2 + y.numel() + w.numel()),
                                                 flops, x.device):
    if bn is None:
      wp = torch.empty(lib().mode_conv1x1_wpack_bytes(Ci, Co) // 4, dtype=torch.float32, device=x.device)
      _call('mode_conv1x1_fwd', ptr(x), ptr(w), ptr(y), ptr(wp), B, Ci, H, W, Co, stride, stream_of(x))
    else:
      e, keep = _epilogue(bn, add, relu, y)
      wp, reuse = _eval_wpack(bn, 'conv1x1_fwd_bn', w, lib().mode_conv1x1_wpack_bytes(Ci, Co) // 4, x.device)
      with reuse:
        _call('mode_conv1x1_fwd_bn', ptr(x), ptr(w), ctypes.byref(e), ptr(y), ptr(wp), B, Ci, H, W, Co, stride, stream_of(x))
  return y


class Conv1x1Function(torch.autograd.Function):

  @staticmethod
  def forward(ctx, x, w, stride):
    ctx.save_for_backward(x, w)
    ctx.stride = stride
    return conv1x1_fwd(x, w, stride)

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, gy):
    x, w = ctx.saved_tensors
    x, w, gy = x.contiguous(), w.contiguous(), gy.contiguous()
    B, Ci, H, W = x.shape
    Co, s = w.shape[0], ctx.stride
    gx = None
    if ctx.needs_input_grad[0]:
      gx = torch.empty_like(x)
      with torch.cuda.device_of(x), profiling.region(_tag1('conv1x1_bwd_data', Ci, Co, s, H, W), 4 * (gx.numel() + gy.numel() + w.numel()),
                                                     2 * gy.numel() * Ci, x.device):
        wp = torch.empty(lib().mode_conv1x1_wpack_bytes(Ci, Co) // 4, dtype=torch.float32, device=x.device)
        _call('mode_conv1x1_bwd_data', ptr(gy), ptr(w), ptr(gx), ptr(wp), B, Ci, H, W, Co, s, stream_of(x))
    gw = None
    if ctx.needs_input_grad[1]:
      sink = grad_sink(w)
      gw = sink if sink is not None else torch.empty_like(w)
      with torch.cuda.device_of(x), profiling.region(_tag1('conv1x1_bwd_weight', Ci, Co, s, H, W), 4 * (x.numel() // s**2 + gy.numel() + w.numel()),
                                                     2 * gy.numel() * Ci, x.device):
        ws = torch.empty(max(lib().mode_conv1x1_bwd_weight_workspace_bytes(B, Ci, H, W, Co, s) // 4, 1), dtype=torch.float32, device=x.device)
        _call('mode_conv1x1_bwd_weight', ptr(gy), ptr(x), ptr(gw), ptr(ws), B, Ci, H, W, Co, s, int(sink is not None), stream_of(x))
      if sink is not None:
        gw = None
    return gx, gw, None


def conv1x1(x, conv):
  return Conv1x1Function.apply(x, conv.weight, conv.stride[0])


# ------------------------------------------------------------------------------------ the 7x7 stride-2 stem (3 -> 32)
def conv_stem_supported(x, conv):
  """firstconv[0] (submodule.py:155): Conv2d(3, <= 32, 7, stride 2, padding 3), on an input that needs no gradient."""
  return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and conv.kernel_size == (7, 7) and conv.stride == (2, 2) and
          conv.padding == (3, 3) and conv.dilation == (1, 1) and conv.groups == 1 and conv.bias is None and conv.in_channels == 3 and
          conv.out_channels <= 32 and conv.padding_mode == 'zeros' and not (torch.is_grad_enabled() and x.requires_grad) and
          32 * x.shape[2] * x.shape[3] < 2**31)


def conv_stem_fwd(x, w, bn=None, add=None, relu=False):
  require_gpu(x, w)
  x, w = x.contiguous(), w.detach().contiguous() if bn is not None else w.contiguous()
  require_f32c(x, w)
  B, Ci, H, W = x.shape
  Co = w.shape[0]
  y = torch.empty((B, Co, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=x.dtype, device=x.device)
  with torch.cuda.device_of(x), profiling.region(_tag1('conv_stem_fwd', Ci, Co, 2, H, W), 4 * (x.numel() + y.numel() + w.numel()),
                                                 2 * y.numel() * Ci * 49, x.device):
    if bn is None:
      wp = torch.empty(lib().mode_conv_stem_wpack_bytes(Ci, Co) // 4, dtype=torch.float32, device=x.device)
      _call('mode_conv_stem_fwd', ptr(x), ptr(w), ptr(y), ptr(wp), B, Ci, H, W, Co, stream_of(x))
    else:
      e, keep = _epilogue(bn, add, relu, y)
      wp, reuse = _eval_wpack(bn, 'conv_stem_fwd_bn', w, lib().mode_conv_stem_wpack_bytes(Ci, Co) // 4, x.device)
      with reuse:
        _call('mode_conv_stem_fwd_bn', ptr(x), ptr(w), ctypes.byref(e), ptr(y), ptr(wp), B, Ci, H, W, Co, stream_of(x))
  return y


class ConvStemFunction(torch.autograd.Function):

  @staticmethod
  def forward(ctx, x, w):
    ctx.save_for_backward(x, w)
    return conv_stem_fwd(x, w)

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, gy):
    x, w = ctx.saved_tensors
    if ctx.needs_input_grad[0]:
      raise RuntimeError('conv_stem: the stem kernels have no input gradient (conv_stem_supported excludes such inputs)')
    gw = None
    if ctx.needs_input_grad[1]:
      x, gy = x.contiguous(), gy.contiguous()
      B, Ci, H, W = x.shape
      Co = w.shape[0]
      sink = grad_sink(w)
      gw = sink if sink is not None else torch.empty_like(w)
      with torch.cuda.device_of(x), profiling.region(_tag1('conv_stem_bwd_weight', Ci, Co, 2, H, W), 4 * (x.numel() + gy.numel() + w.numel()),
                                                     2 * gy.numel() * Ci * 49, x.device):
        ws = torch.empty(max(lib().mode_conv_stem_bwd_weight_workspace_bytes(B, Ci, H, W, Co) // 4, 1), dtype=torch.float32, device=x.device)
        _call('mode_conv_stem_bwd_weight', ptr(gy), ptr(x), ptr(gw), ptr(ws), B, Ci, H, W, Co, int(sink is not None), stream_of(x))
      if sink is not None:
        gw = None
    return None, gw


def conv_stem(x, conv):
  return ConvStemFunction.apply(x, conv.weight)


# ------------------------------------------------------------------------------------ any other Conv2d: gather-and-MAC on an integer table
# The extractor's remaining regular convolutions -- 7x7 stride 2 (stem), 3x3 stride 2, 1x1 (stride 1 and 2); submodule.py:155,
# 158, 162, 167-174 -- are the spherical operator with an INTEGER sampling table: tap (i, j) of output pixel (h, w) reads input
# pixel (h*s + i*d - p, w*s + j*d - p), the bilinear weights are exactly (1, 0, 0, 0) and positions outside the image are dropped
# by the operator's own guard (cu:246), which is zero padding.  Same kernels as SphereConv (general gather-and-MAC forward,
# adjoint-gather input gradient, split-K weight gradient), bit-for-bit a plain convolution up to the order of the fp32 sums.
_conv_tables = _LRU(TABLE_CACHE_ENTRIES)
_conv_table_lock = threading.Lock()


MAX_TAPS = 32  # tap limit of the general gather-and-MAC kernels (csrc/sphere_conv.hip)


def conv2d_table(H, W, kh, kw, stride, pad, dil, device, row0=0):
  """(1, 2*kh*kw, H, W) float32 table on `device`: channel 2k = row, 2k+1 = column read by tap k = (i, j) at the output pixel
  whose top-left input position is (h, w) (the operator samples it at (h_out*stride, w_out*stride), cu:206-261); tap rows are
  numbered from `row0` (a kernel with more than MAX_TAPS taps runs as several row bands).  Cached."""
  key = (H, W, kh, kw, tuple(stride), tuple(pad), tuple(dil), str(device), row0)
  with _conv_table_lock:
    t = _conv_tables.get(key)
    if t is None:
      hh = torch.arange(H, dtype=torch.float32).view(H, 1).expand(H, W)
      ww = torch.arange(W, dtype=torch.float32).view(1, W).expand(H, W)
      planes = []
      for i in range(row0, row0 + kh):
        for j in range(kw):
          planes += [hh + float(i * dil[0] - pad[0]), ww + float(j * dil[1] - pad[1])]
      t = _conv_tables[key] = torch.stack(planes, 0).unsqueeze(0).contiguous().to(device)
    return t


def conv2d_tabled_supported(x, conv):
  """The operator reads its table at (h_out * stride, w_out * stride): the output grid must fit into the input grid (any 'same'
  or shrinking geometry; a convolution padded beyond that stays with the vendor library)."""
  if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and conv.groups == 1 and conv.bias is None and
          conv.padding_mode == 'zeros' and not isinstance(conv.padding, str) and conv.kernel_size[1] <= MAX_TAPS and
          x.shape[2] >= conv.kernel_size[0] and x.shape[3] >= conv.kernel_size[1]):
    return False
  for n, k, s, p, d in zip(x.shape[2:], conv.kernel_size, conv.stride, conv.padding, conv.dilation):
    out = (n + 2 * p - (d * (k - 1) + 1)) // s + 1
    if out < 1 or (out - 1) * s > n - 1:
      return False
  return True


def _row_bands(kh, kw):
  """[(first row, rows)] with rows * kw <= MAX_TAPS each: 3x3 -> [(0, 3)], 7x7 -> [(0, 4), (4, 3)]."""
  per = max(1, MAX_TAPS // kw)
  return [(r, min(per, kh - r)) for r in range(0, kh, per)]


class Conv2dTabledFunction(torch.autograd.Function):

  @staticmethod
  def forward(ctx, x, w, stride, pad, dil):
    x, w = x.contiguous(), w.contiguous()
    B, Ci, H, W = x.shape
    Co, _, kh, kw = w.shape
    Ho = (H + 2 * pad[0] - (dil[0] * (kh - 1) + 1)) // stride[0] + 1
    Wo = (W + 2 * pad[1] - (dil[1] * (kw - 1) + 1)) // stride[1] + 1
    y = torch.empty((B, Co, Ho, Wo), dtype=x.dtype, device=x.device)
    bands = _row_bands(kh, kw)
    for r0, rows in bands:
      pos = conv2d_table(H, W, rows, kw, stride, pad, dil, x.device, r0)
      if len(bands) == 1:
        sphere_conv_fwd(x, pos, w, y, stride, 1)
      else:  # y = sum over the row bands of the kernel
        part = y if r0 == 0 else torch.empty_like(y)
        sphere_conv_fwd(x, pos, w[:, :, r0:r0 + rows].contiguous(), part, stride, 1)
        if r0:
          y += part
    ctx.save_for_backward(x, w)
    ctx.geom = (tuple(stride), tuple(pad), tuple(dil))
    return y

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, gy):
    x, w = ctx.saved_tensors
    stride, pad, dil = ctx.geom
    H, W = x.shape[2:]
    kh, kw = w.shape[2:]
    gy = gy.contiguous()
    bands = _row_bands(kh, kw)
    gx = None
    if ctx.needs_input_grad[0]:
      gx = torch.empty_like(x)
      for r0, rows in bands:
        pos = conv2d_table(H, W, rows, kw, stride, pad, dil, x.device, r0)
        if len(bands) == 1:
          sphere_conv_bwd_data(gy, pos, w, gx, stride, 1, overwrite=True)
        else:
          part = gx if r0 == 0 else torch.empty_like(gx)
          sphere_conv_bwd_data(gy, pos, w[:, :, r0:r0 + rows].contiguous(), part, stride, 1, overwrite=True)
          if r0:
            gx += part
    gw = None
    if ctx.needs_input_grad[1]:
      sink = grad_sink(w)
      gw = sink if sink is not None else torch.zeros_like(w)
      for r0, rows in bands:
        pos = conv2d_table(H, W, rows, kw, stride, pad, dil, x.device, r0)
        if len(bands) == 1:
          sphere_conv_bwd_weight(gy, pos, x, gw, stride, 1)
        else:
          part = torch.zeros((w.shape[0], w.shape[1], rows, kw), dtype=w.dtype, device=w.device)
          sphere_conv_bwd_weight(gy, pos, x, part, stride, 1)
          gw[:, :, r0:r0 + rows] += part
      if sink is not None:
        gw = None
    return gx, gw, None, None, None


def conv2d_tabled(x, conv):
  """nn.Conv2d `conv` (any kernel size / stride / padding / dilation; groups 1, no bias) on the gather-and-MAC kernels."""
  return Conv2dTabledFunction.apply(x, conv.weight, tuple(conv.stride), tuple(conv.padding), tuple(conv.dilation))


# ------------------------------------------------------------------------------------ gradient sinks
def grad_sink(param):
  """The buffer parameter gradients are accumulated into directly by the native backward kernels, or None.

  autograd's AccumulateGrad costs one extra elementwise kernel per parameter and step (243 launches for ModeDisparity).
  When a parameter carries `_mode_grad_sink` (set by data_parallel.GradAllReducer: a view into its flat gradient buffer,
  which is also `param.grad`), the weight-gradient kernels add into that view themselves and the autograd Function
  returns None for the parameter, so nothing is left for autograd to accumulate.  Parameters without the attribute get
  ordinary autograd gradients."""
  sink = getattr(param, '_mode_grad_sink', None)
  if sink is None:
    return None
  if param.grad is None or param.grad.data_ptr() != sink.data_ptr():
    # optimizer.zero_grad() (set_to_none=True by default; train_disparity.py:149) or anything else replaced .grad: adding into
    # the detached buffer would silently drop this parameter's gradient, so autograd accumulates it the ordinary way
    # (GradAllReducer.rebind() re-attaches the views)
    return None
  if not (sink.is_cuda and sink.dtype == torch.float32 and sink.is_contiguous() and sink.shape == param.shape):
    raise RuntimeError('gradient sink of a %s parameter must be a contiguous fp32 device tensor of the same shape' % (tuple(param.shape),))
  return sink


# ------------------------------------------------------------------------------------ tensors with several consumers
def sum_n(tensors):
  """a + b [+ c [+ d]] in one pass (mode_sum_n); more than four operands in groups of four."""
  ts = [t.contiguous() for t in tensors]
  require_gpu(*ts)
  require_f32c(*ts)
  while len(ts) > 1:
    grp, ts = ts[:4], ts[4:]
    out = torch.empty_like(grp[0])
    with torch.cuda.device_of(out), profiling.region('grad_sum%d' % len(grp), 4 * out.numel() * (len(grp) + 1), 0, out.device):
      _call('mode_sum_n', ptr(grp[0]), ptr(grp[1]), ptr(grp[2]) if len(grp) > 2 else None, ptr(grp[3]) if len(grp) > 3 else None, ptr(out),
            out.numel(), stream_of(out))
    ts = [out] + ts
  return ts[0]


class FanOutFunction(torch.autograd.Function):
  """n aliases of x, one per consumer.  autograd would accumulate the consumers' gradients pairwise (n - 1 launches, each reading two
  tensors and writing one); here they arrive together and are summed in ONE pass.  Pays from three consumers on: cost0 (the input of
  dres2 and three residual adds) and pre1 (mode_disparity.py:119-125); exact up to the association of the fp32 sum."""

  @staticmethod
  def forward(ctx, x, n):
    return tuple(x.view_as(x) for _ in range(n))

  @staticmethod
  def backward(ctx, *grads):
    live = [g for g in grads if g is not None]
    if not live:
      return None, None
    return (live[0] if len(live) == 1 else sum_n(live)), None


# A tensor with exactly TWO consumers whose gradients autograd would add in a separate pass (read two tensors, write one): the consumer
# whose backward runs first leaves its gradient in the carrier and reports None, the second adds it inside the kernel that produces its
# own (mode_conv3d_bwd_data_split_acc: one extra read in the store instead of three passes) -- the same fp32 sum, bit for bit.  Both
# consumers register in their forward (arm); a gradient is only left behind when both did.  Consumers that cannot add in their kernel
# (the BatchNorm backward that owns a residual skip's gradient) can still be the first.
# The hand-off relies on both backwards running in the same pass -- what this model's training step guarantees -- and CHECKS it (ADVICE
# r5): the consumer that leaves a gradient queues a callback for the end of that backward pass; a gradient still parked then means the
# partner never ran (backward(inputs=...), autograd.grad on a sub-graph): the pass has reported None for a gradient it dropped, and
# the callback raises instead of letting a wrong gradient through (and un-parks the tensor, up to 403 MB).  A gradient left over from a
# pass that died before its callbacks ran is recognised by its owner -- the same consumer asking first again -- and dropped.
GRAD_CARRIERS = True  # bench.py --no-grad-carriers measures autograd's own accumulation


class GradCarrier(object):
  __slots__ = ('armed', 'grad', 'owner')

  def __init__(self):
    self.armed = 0
    self.grad = None
    self.owner = None

  def arm(self, needs_grad):
    if needs_grad:
      self.armed += 1

  def take(self, who=None):
    """The partner's gradient when it came first, else None.  `who` identifies the asking consumer (its autograd ctx): a gradient it
    parked itself is a leftover of an earlier, aborted pass -- dropped, not added."""
    g, owner = self.grad, self.owner
    self.grad = self.owner = None
    if g is not None and who is not None and owner is who:
      return None
    return g

  def leave(self, g, who=None):
    """First of the two backwards: True when g was left for the other one (report None to autograd), False to return it as usual."""
    if self.armed == 2 and g is not None:
      self.grad, self.owner = g, who
      try:
        torch.autograd.Variable._execution_engine.queue_callback(self._end_of_pass)
      except RuntimeError:  # (not inside a backward pass: nothing to check against; behave like autograd)
        self.grad = self.owner = None
        return False
      return True
    return False

  def _end_of_pass(self):
    if self.grad is not None:
      self.grad = self.owner = None
      raise RuntimeError('mode_hip GradCarrier: one of the two consumers of a shared tensor ran its backward and the other did not '
                         '(backward(inputs=...) / autograd.grad on a sub-graph?): the gradient of the shared tensor would be incomplete. '
                         'Set mode_hip.functional.GRAD_CARRIERS = False for partial backward passes.')


def grad_carrier(x):
  """A carrier for tensor x, or None when nothing would be gained (no gradient needed, CPU tensor, switched off)."""
  return GradCarrier() if (GRAD_CARRIERS and x.is_cuda and x.dtype == torch.float32 and torch.is_grad_enabled() and x.requires_grad) else None


def fan_out(x, n):
  if n <= 1 or not (x.is_cuda and x.dtype == torch.float32 and torch.is_grad_enabled() and x.requires_grad):
    return (x,) * max(n, 1)
  return FanOutFunction.apply(x, n)


# ------------------------------------------------------------------------------------ 3x3x3 convolution / transposed conv
def _wpack3d(ci, co, device):
  n = lib().mode_conv3d_wpack_bytes(ci, co)
  return torch.empty(n // 4, dtype=torch.float32, device=device)


# Arithmetic of the 3x3(x3) stride-1 convolution layers -- the 3D regulariser's stride-1 layers (forward, input gradient, weight
# gradient), the extractor's regular 3x3 Conv2d layers (all three) and the forward of its spherical layers (small-window tiles):
#   'bf16x6' (default) fp32 operands split EXACTLY into three bf16 pieces when a tile is staged, six bf16 MFMAs per product (the
#            terms >= 2^-16 of it), fp32 accumulation (csrc/conv3d_split.hip, conv3d_split_wgrad.hip, conv2d_split.hip).  Results carry
#            the rounding of an fp32 convolution -- measured against float64 they are at least as close as the fp32 MFMA kernels' on
#            the same inputs (tests/test_gpu_split.py) -- at 1.5-2 x their speed.  Layers the split kernels do not cover (stride 2,
#            transposed, single-channel heads, channel counts off their grid) run on the fp32 kernels.
#   'f32'    v_mfma_f32_32x32x2_f32 everywhere (csrc/conv3d_f32_fwd.hip, conv3d_f32_wgrad.hip, conv2d_f32_fwd.hip, conv2d_f32_wgrad.hip).
# Process-wide, read at call time (bench.py --conv-arith; the parity tests run under both).
CONV_ARITH = 'bf16x6'


def set_conv_arith(kind):
  global CONV_ARITH
  if kind not in ('f32', 'bf16x6'):
    raise ValueError("convolution arithmetic must be 'f32' or 'bf16x6', got %r" % (kind,))
  CONV_ARITH = kind


def _split3d(ci, co, stride, which, vol=None):
  """which: 0 forward, 1 input gradient, 2 weight gradient.  vol = (D, H, W) of the convolution's input: the layer runs on the split
  kernel AT THIS SIZE (mode_conv3d_split_shape_supported: the channel counts and every 32-bit contract of the kernel, csrc/size_contracts.h;
  a volume beyond them runs on the fp32 kernel instead of failing).  Without vol: the channel counts alone."""
  if CONV_ARITH != 'bf16x6':
    return False
  if vol is None:
    return lib().mode_conv3d_split_supported(ci, co, stride, int(which)) == 1
  return lib().mode_conv3d_split_shape_supported(ci, co, int(vol[0]), int(vol[1]), int(vol[2]), stride, int(which)) == 1


def _deconv_split3d(cin, cout, vol):
  """The transposed convolution (cin, D, H, W) -> (cout, 2D, 2H, 2W) on the split kernel: it is the input gradient of the stride-2
  convolution cout -> cin over the doubled volume."""
  return _conv3d_route(cout, cin, 2, 1, (2 * vol[0], 2 * vol[1], 2 * vol[2]), False) == 's2_split'


def _out3(n, stride):
  return (n - 1) // stride + 1


def _tag3(name, ci, co, stride, d, h, w):
  """Profiling label carrying the layer shape (input volume of the convolution), e.g. conv3d_fwd[32->32 s1 48x256x128]."""
  return '%s[%d->%d s%d %dx%dx%d]' % (name, ci, co, stride, d, h, w) if profiling.ENABLED else name


# Two fp16 pieces and three MFMAs per product (mode_conv3d_*_split_f16) for the stride-1 3-D layers that the split kernels
# cover: each operand scaled by a power of two taken from its tensor's largest finite magnitude -- left by the pass that wrote the tensor
# (the `_amax` entries), or by mode_abs_max.  One switch per kind of call, each on by default and read at call time; _conv3d_route gets the
# one that applies as its `f16` argument:
#   CONV3D_S1_F16    a TRAINING step's forward and both gradients (`bench.py --no-conv3d-f16` is the A/B);
#   CONV3D_EVAL_F16  an INFERENCE forward (conv3d_bn_eval: the folded-BatchNorm epilogues on the same arithmetic, the activations' maxima
#                    out of the kernels' epilogues; mode_conv3d_fwd_split_f16_bn), and
#   CONV2D_EVAL_F16  the extractor's stride-1 3 x 3 layers of an inference forward (mode_conv2d_fwd_split_f16_bn; _conv2d_route).
# Precision contract (stated once in csrc/split_arith.h; include/mode_hip.h for the entries): on two fp16 pieces an element keeps 22
# significant bits down to ~2^-17 of its tensor's maximum, fewer below, none below ~2^-39 of it -- in training AND, by default, in
# inference.  With a switch set to False its calls run on three bf16 pieces, which keep 24 bits of every element whatever its size: set
# both *_EVAL_F16 globals to False before the forward to keep inference there (`bench.py --no-eval-f16` does exactly that).
CONV3D_S1_F16 = True
CONV3D_EVAL_F16 = True
CONV2D_EVAL_F16 = True


BN_ABSMAX_FLOATS = CONSTANTS['MODE_BN_ABSMAX_FLOATS']  # the buffer a tensor's maximum lives in


def abs_max(t):
  """The largest finite magnitude in t as the fp16-arithmetic kernels take it (mode_abs_max; no host synchronisation): a device buffer
  of BN_ABSMAX_FLOATS floats whose maximum is the value (abs_max_value reads it on the host).  A tensor's maximum is computed once and
  handed to every kernel that reads the tensor (the forward's x again in the weight gradient, gy in both gradients)."""
  out = torch.empty(BN_ABSMAX_FLOATS, dtype=torch.float32, device=t.device)
  _call('mode_abs_max', ptr(t), t.numel(), ptr(out), stream_of(t))
  return out


def abs_max_value(buf):
  """Host value of a maximum buffer (abs_max, known_abs_max): its entries are non-negative floats, the value is their maximum.  Synchronises."""
  return float(buf.max())


def _conv3d_route(ci, co, stride, which, vol, f16):
  """The kernel family of the 3x3x3 layer ci -> co (stride 1 | 2) at the input volume vol = (D, H, W) -- which: 0 forward, 1 input
  gradient, 2 weight gradient:
    'f32'        the fp32 MFMA kernels: CONV_ARITH 'f32', channel counts off the split kernels' grid, or a volume beyond their 32-bit
                 contracts (_split3d);
    's2_split'   stride 2 on three bf16 pieces;
    'split_f16'  stride 1 on two fp16 pieces -- where f16: a training call passes CONV3D_S1_F16, the inference wrapper CONV3D_EVAL_F16;
    'split'      stride 1 on three bf16 pieces."""
  if not _split3d(ci, co, stride, which, vol):
    return 'f32'
  if stride == 2:
    return 's2_split'
  return 'split_f16' if f16 else 'split'


def conv3d_s1_f16(ci, co, which, vol=None):
  """True when the stride-1 layer ci -> co runs its forward (which 0) / input gradient (1) / weight gradient (2) on the fp16 arithmetic
  (vol = (D, H, W): at this size)."""
  return _conv3d_route(ci, co, 1, which, vol, CONV3D_S1_F16) == 'split_f16'


def conv3d_fwd(x, w, stride=1, amax=None):
  """x (B,Ci,D,H,W), w (Co,Ci,3,3,3) -> (B,Co,Do,Ho,Wo); k3 p1, stride 1|2, no bias (convbn_3d, submodule.py:20-22).
  amax = (max |x|, max |w|) device scalars when the caller has them (fp16 arithmetic only; computed here otherwise)."""
  require_gpu(x, w)
  x, w = x.contiguous(), w.contiguous()
  require_f32c(x, w)
  B, Ci, D, H, W = x.shape
  Co = w.shape[0]
  if tuple(w.shape[1:]) != (Ci, 3, 3, 3):
    raise RuntimeError('conv3d: weight %s does not match input channels %d / kernel 3' % (tuple(w.shape), Ci))
  y = torch.empty((B, Co, _out3(D, stride), _out3(H, stride), _out3(W, stride)), dtype=x.dtype, device=x.device)
  flops = 2 * y.numel() * Ci * 27
  with torch.cuda.device_of(x), profiling.region(_tag3('conv3d_fwd', Ci, Co, stride, D, H, W), 4 * (x.numel() + y.numel() + w.numel()),
                                                 flops, x.device):
    wp = _wpack3d(Ci, Co, x.device)
    route = _conv3d_route(Ci, Co, stride, 0, (D, H, W), CONV3D_S1_F16)
    tail = (ptr(y), ptr(wp), B, Ci, D, H, W, Co)
    if route == 'split_f16':
      ax, aw = amax if amax is not None else (abs_max(x), abs_max(w))
      _call('mode_conv3d_fwd_split_f16', ptr(x), ptr(w), ptr(ax), ptr(aw), *tail, stream_of(x))
    elif route == 'f32':
      _call('mode_conv3d_fwd', ptr(x), ptr(w), *tail, stride, stream_of(x))
    else:  # (None: no folded-BatchNorm epilogue)
      _call('mode_conv3d_fwd_s2_split' if route == 's2_split' else 'mode_conv3d_fwd_split', ptr(x), ptr(w), None, *tail, stream_of(x))
  return y


def conv3d_bwd_data(gy, w, in_shape, stride=1, acc=None, amax=None):
  """gradient w.r.t. the input of conv3d_fwd; in_shape = x.shape.  acc: a gradient of the same tensor that is already there -- the sum
  is returned (added in the kernel's store on the split path, by a separate pass elsewhere)."""
  require_gpu(gy, w)
  gy, w = gy.contiguous(), w.contiguous()
  require_f32c(gy, w)
  B, Ci, D, H, W = in_shape
  Co = w.shape[0]
  gx = torch.empty((B, Ci, D, H, W), dtype=gy.dtype, device=gy.device)
  flops = 2 * gy.numel() * Ci * 27
  route = _conv3d_route(Ci, Co, stride, 1, (D, H, W), CONV3D_S1_F16)
  in_store = False  # acc is an argument of the chosen entry (one more tensor read in its store); else gx.add_(acc) behind it
  if acc is not None:
    acc = acc.contiguous()
    in_store = (tuple(acc.shape) == tuple(gx.shape) and acc.dtype == gx.dtype and route != 'f32' and
                lib().mode_conv3d_bwd_data_split_acc_supported(Ci, Co, stride) == 1)
  with torch.cuda.device_of(gy), profiling.region(_tag3('conv3d_bwd_data', Ci, Co, stride, D, H, W),
                                                  4 * ((2 if in_store else 1) * gx.numel() + gy.numel() + w.numel()), flops, gy.device):
    wp = _wpack3d(Ci, Co, gy.device)
    tail = (ptr(gx), ptr(wp), B, Ci, D, H, W, Co)
    if route == 'split_f16':
      ag, aw = amax if amax is not None else (abs_max(gy), abs_max(w))
      _call('mode_conv3d_bwd_data_split_f16', ptr(gy), ptr(w), ptr(ag), ptr(aw), ptr(acc) if in_store else None, *tail, stream_of(gy))
    elif in_store:  # ('split' and 's2_split' alike)
      _call('mode_conv3d_bwd_data_split_acc', ptr(gy), ptr(w), ptr(acc), *tail, stride, stream_of(gy))
    elif route == 'f32':
      _call('mode_conv3d_bwd_data', ptr(gy), ptr(w), *tail, stride, stream_of(gy))
    else:
      _call('mode_conv3d_bwd_data_s2_split' if route == 's2_split' else 'mode_conv3d_bwd_data_split', ptr(gy), ptr(w), *tail, stream_of(gy))
  return gx if acc is None or in_store else gx.add_(acc)


def conv3d_bwd_weight(gy, x, stride=1, into=None, amax=None):
  """gW (Co,Ci,3,3,3) = sum gy[o, q] * x[c, stride*q + k - 1]; returned, or ADDED to `into` when given.
  amax = (max |gy|, max |x|) device scalars when the caller has them (fp16 arithmetic only)."""
  require_gpu(gy, x)
  gy, x = gy.contiguous(), x.contiguous()
  require_f32c(gy, x)
  B, Ci, D, H, W = x.shape
  Co = gy.shape[1]
  gw = into if into is not None else torch.empty((Co, Ci, 3, 3, 3), dtype=gy.dtype, device=gy.device)
  if gw.numel() != Co * Ci * 27:
    raise RuntimeError('conv3d_bwd_weight: gradient buffer %s does not hold %dx%dx27 values' % (tuple(gw.shape), Co, Ci))
  flops = 2 * gy.numel() * Ci * 27
  with torch.cuda.device_of(gy), profiling.region(_tag3('conv3d_bwd_weight', Ci, Co, stride, D, H, W),
                                                  4 * (x.numel() + gy.numel() + gw.numel()), flops, gy.device):
    n = lib().mode_conv3d_bwd_weight_workspace_bytes(B, Ci, D, H, W, Co, stride)
    ws = torch.empty(max(n // 4, 1), dtype=torch.float32, device=gy.device)
    route = _conv3d_route(Ci, Co, stride, 2, (D, H, W), CONV3D_S1_F16)
    tail = (ptr(gw), ptr(ws), B, Ci, D, H, W, Co)
    if route == 'split_f16':
      ag, ax = amax if amax is not None else (abs_max(gy), abs_max(x))
      _call('mode_conv3d_bwd_weight_split_f16', ptr(gy), ptr(x), ptr(ag), ptr(ax), *tail, int(into is not None), stream_of(gy))
    elif route == 'f32':
      _call('mode_conv3d_bwd_weight', ptr(gy), ptr(x), *tail, stride, int(into is not None), stream_of(gy))
    else:
      _call('mode_conv3d_bwd_weight_s2_split' if route == 's2_split' else 'mode_conv3d_bwd_weight_split', ptr(gy), ptr(x), *tail,
            int(into is not None), stream_of(gy))
  return gw


def deconv3d_fwd(x, w):
  """ConvTranspose3d k3 s2 p1 op1: x (B,Cin,D,H,W), w (Cin,Cout,3,3,3) -> (B,Cout,2D,2H,2W) (mode_disparity.py:23, 25)."""
  require_gpu(x, w)
  x, w = x.contiguous(), w.contiguous()
  require_f32c(x, w)
  B, Cin, D, H, W = x.shape
  Cout = w.shape[1]
  if w.shape[0] != Cin or tuple(w.shape[2:]) != (3, 3, 3):
    raise RuntimeError('deconv3d: weight %s does not match input channels %d / kernel 3' % (tuple(w.shape), Cin))
  y = torch.empty((B, Cout, 2 * D, 2 * H, 2 * W), dtype=x.dtype, device=x.device)
  flops = 2 * x.numel() * Cout * 27
  with torch.cuda.device_of(x), profiling.region('deconv3d_fwd', 4 * (x.numel() + y.numel() + w.numel()), flops, x.device):
    wp = _wpack3d(Cin, Cout, x.device)
    _call('mode_deconv3d_fwd_split' if _deconv_split3d(Cin, Cout, (D, H, W)) else 'mode_deconv3d_fwd', ptr(x), ptr(w), ptr(y), ptr(wp), B, Cin,
          D, H, W, Cout, stream_of(x))
  return y


class Conv3dFunction(torch.autograd.Function):
  """k3 p1 convolution (stride 1|2) on the HIP kernels; autograd of F.conv3d(x, w, None, stride, 1)."""

  @staticmethod
  def forward(ctx, x, w, stride, carrier=None):
    ctx.save_for_backward(x, w)
    ctx.stride = stride
    ctx.carrier = carrier  # GradCarrier of x (x has one other consumer), or None
    ctx.amax = None
    if x.is_cuda and _conv3d_route(x.shape[1], w.shape[0], stride, 0, x.shape[2:], CONV3D_S1_F16) == 'split_f16':
      ax = known_abs_max(x)  # left by the BatchNorm pass that wrote x, where there is one
      ctx.amax = (ax if ax is not None else abs_max(x.contiguous()), _weight_abs_max(w.contiguous()))  # the backward reads both tensors again
    return conv3d_fwd(x, w, stride, amax=ctx.amax)

  @staticmethod
  def backward(ctx, gy):
    x, w = ctx.saved_tensors
    gx = None
    fwd_amax = getattr(ctx, 'amax', None)
    ag = None
    if fwd_amax is not None:  # fp16 arithmetic: gy's maximum once, for both gradients
      ag = known_abs_max(gy)  # left by the BatchNorm backward that wrote gy, where that is where gy comes from
      gy = gy.contiguous()
      if ag is None:
        ag = abs_max(gy)
    if ctx.needs_input_grad[0]:
      carrier = getattr(ctx, 'carrier', None)  # (Conv3dStatsFunction shares this backward and has none)
      prev = carrier.take(ctx) if carrier is not None else None  # the other consumer's gradient, when it came first
      gx = conv3d_bwd_data(gy, w, x.shape, ctx.stride, acc=prev, amax=(ag, fwd_amax[1]) if ag is not None else None)
      if prev is None and carrier is not None and carrier.leave(gx, ctx):
        gx = None  # first of the two: the other consumer's backward returns the sum
    gw = None
    if ctx.needs_input_grad[1]:
      sink = grad_sink(w)
      gw = conv3d_bwd_weight(gy, x, ctx.stride, into=sink, amax=(ag, fwd_amax[0]) if ag is not None else None)
      if sink is not None:
        gw = None
    return gx, gw, None, None


class Deconv3dFunction(torch.autograd.Function):
  """ConvTranspose3d k3 s2 p1 op1; its input gradient is a stride-2 convolution with the same weights and its weight
  gradient the stride-2 weight-gradient kernel with the roles of input and output gradient exchanged."""

  @staticmethod
  def forward(ctx, x, w):
    ctx.save_for_backward(x, w)
    return deconv3d_fwd(x, w)

  @staticmethod
  def backward(ctx, gy):
    x, w = ctx.saved_tensors
    gx = conv3d_fwd(gy, w, 2) if ctx.needs_input_grad[0] else None  # w (Cin,Cout,27) read as (Co=Cin, Ci=Cout)
    gw = None
    if ctx.needs_input_grad[1]:
      sink = grad_sink(w)
      gw = conv3d_bwd_weight(x, gy, 2, into=sink)  # -> (Cin, Cout, 3,3,3)
      if sink is not None:
        gw = None
    return gx, gw


def conv3d(x, w, stride=1, carrier=None):
  if carrier is not None:
    carrier.arm(x.requires_grad and torch.is_grad_enabled())
  return Conv3dFunction.apply(x, w, stride, carrier)


# BatchNorm statistics in the epilogue of the stride-1 split 3-D convolution (training) instead of a statistics pass over its output.
# Built and measured in round 4 (same box, graph-replayed step): the ten BatchNorm layers behind these convolutions get 0.41 ms
# cheaper, the convolution launches 0.36 ms dearer (0.78 -> 0.82 ms at 32 -> 32 / 48 x 256 x 128: the tile epilogue of a persistent,
# one-workgroup-per-CU kernel is not overlapped with anything, so whatever is added to it is paid in full): 73.03-73.41 against
# 73.17-73.39 ms per step.  Off by default -- the two-kernel path has one code path fewer; `bench.py --fused-bn-stats` measures it.
CONV3D_BN_STATS = False


def conv3d_stats_supported(x, w, bn):
  """Training-mode convbn_3d whose stride-1 convolution runs on the split kernel: the BatchNorm batch statistics can be taken in the
  convolution's epilogue (mode_conv3d_fwd_split_stats) instead of by a pass over its output."""
  return (CONV3D_BN_STATS and x.is_cuda and x.dtype == torch.float32 and x.dim() == 5 and x.shape[0] > 0 and bn.training and
          bn.momentum is not None and _conv3d_route(x.shape[1], w.shape[0], 1, 0, x.shape[2:], False) == 'split' and
          x.shape[0] * w.shape[0] < 65536)


class Conv3dStatsFunction(torch.autograd.Function):
  """Conv3dFunction (stride 1) that also fills `ws` -- the workspace of the BatchNorm that follows -- with the batch statistics of its
  output (partial sums per workgroup + pivots).  `ws` is a plain buffer, not differentiable."""

  @staticmethod
  def forward(ctx, x, w, ws):
    require_gpu(x, w, ws)
    x, w = x.contiguous(), w.contiguous()
    require_f32c(x, w, ws)
    B, Ci, D, H, W = x.shape
    Co = w.shape[0]
    if tuple(w.shape[1:]) != (Ci, 3, 3, 3):
      raise RuntimeError('conv3d: weight %s does not match input channels %d / kernel 3' % (tuple(w.shape), Ci))
    y = torch.empty((B, Co, D, H, W), dtype=x.dtype, device=x.device)
    with torch.cuda.device_of(x), profiling.region(_tag3('conv3d_fwd', Ci, Co, 1, D, H, W), 4 * (x.numel() + y.numel() + w.numel()),
                                                   2 * y.numel() * Ci * 27, x.device):
      wp = _wpack3d(Ci, Co, x.device)
      _call('mode_conv3d_fwd_split_stats', ptr(x), ptr(w), ptr(y), ptr(wp), ptr(ws), B, Ci, D, H, W, Co, stream_of(x))
    ctx.save_for_backward(x, w)
    ctx.stride = 1
    return y

  @staticmethod
  def backward(ctx, gy):
    return Conv3dFunction.backward(ctx, gy)[:3]  # (x, w, ws)


def conv3d_bn_train(x, conv_weight, bn, add=None, relu=False):
  """relu?(batch_norm_train(conv3d(x, w, stride 1, padding 1)) [+ add]) with the statistics pass folded into the convolution."""
  ws = _bn_ws(conv_weight.shape[0], x.device)
  update = bn.training and bn.track_running_stats
  y = Conv3dStatsFunction.apply(x, conv_weight, ws)
  nbt = bn.num_batches_tracked if update else None
  if nbt is not None and not (nbt.is_cuda and nbt.dtype == torch.int64):
    nbt.add_(1)
    nbt = None
  return BnActFunction.apply(y, add, bn.weight, bn.bias, bn.running_mean if update else None, bn.running_var if update else None, bn.momentum,
                             bn.eps, relu, nbt, 1, ws)


def deconv3d(x, w):
  return Deconv3dFunction.apply(x, w)


# ------------------------------------------------------------------------------------ fused soft-argmin head
def _tag_head(name, D4, H, W):
  """Profiling label with the shape, e.g. head_bwd[48x1024x512] (nodes along the disparity axis x output height x output width)."""
  return '%s[%dx%dx%d]' % (name, D4, H, W) if profiling.ENABLED else name


def head_fwd(logits, size, with_confidence=False):
  """logits (B,1,D4,H4,W4) -> pred (B,1,H,W) [, conf (B,1,H,W)] for size = (D,H,W).
  Replaces mode_disparity.py:131-152 (+ :157-183 for the confidence map)."""
  require_gpu(logits)
  logits = logits.contiguous()
  require_f32c(logits)
  B, one, D4, H4, W4 = logits.shape
  if one != 1:
    raise ValueError('head: expected (B,1,D/4,H/4,W/4) logits, got %s' % (tuple(logits.shape),))
  D, H, W = size
  pred = torch.empty((B, 1, H, W), dtype=logits.dtype, device=logits.device)
  conf = torch.empty_like(pred) if with_confidence else None
  nbytes = 4 * (logits.numel() + pred.numel() * (2 if with_confidence else 1))
  with torch.cuda.device_of(logits), profiling.region(_tag_head('head_fwd', D4, H, W), nbytes, 0, logits.device):
    _call('mode_head_fwd', ptr(logits), ptr(pred), _optr(conf), B, D4, H4, W4, D, H, W, stream_of(logits))
  return (pred, conf) if with_confidence else pred


def head_bwd(logits, gpred, size):
  require_gpu(logits, gpred)
  logits, gpred = logits.contiguous(), gpred.contiguous()
  require_f32c(logits, gpred)
  B, _, D4, H4, W4 = logits.shape
  D, H, W = size
  gl = torch.empty_like(logits)
  nbytes = 4 * (2 * logits.numel() + gpred.numel())
  with torch.cuda.device_of(logits), profiling.region(_tag_head('head_bwd', D4, H, W), nbytes, 0, logits.device):
    n = lib().mode_head_bwd_workspace_bytes(B, D4, H, W)
    ws = torch.empty(max(n // 4, 1), dtype=torch.float32, device=logits.device)
    _call('mode_head_bwd', ptr(logits), ptr(gpred), ptr(gl), ptr(ws), B, D4, H4, W4, D, H, W, stream_of(logits))
  return gl


class HeadFunction(torch.autograd.Function):

  @staticmethod
  def forward(ctx, logits, size):
    ctx.save_for_backward(logits)
    ctx.size = tuple(size)
    return head_fwd(logits, size)

  @staticmethod
  def backward(ctx, gpred):
    logits, = ctx.saved_tensors
    return head_bwd(logits, gpred, ctx.size), None


def head(logits, size):
  return HeadFunction.apply(logits, size)


def head_bwd_conf(logits, pred, conf, gpred, gconf, size):
  """The gradient of head_fwd(logits, size, with_confidence=True) = (pred, conf) with respect to the logits for the upstream gradients
  (gpred, gconf), in the launches of head_bwd (mode_head_bwd_conf): pred and conf are the forward's own outputs, the rounding that
  places the confidence window passes no gradient."""
  require_gpu(logits, pred, conf, gpred, gconf)
  logits, pred, conf, gpred, gconf = [t.contiguous() for t in (logits, pred, conf, gpred, gconf)]
  require_f32c(logits, pred, conf, gpred, gconf)
  B, _, D4, H4, W4 = logits.shape
  D, H, W = size
  for name, t in (('pred', pred), ('conf', conf), ('gpred', gpred), ('gconf', gconf)):
    if t.numel() != B * H * W:
      raise ValueError('head_bwd_conf: %s %s is not (B, 1, H, W) = %s' % (name, tuple(t.shape), (B, 1, H, W)))
  gl = torch.empty_like(logits)
  nbytes = 4 * (2 * logits.numel() + 4 * gpred.numel())
  with torch.cuda.device_of(logits), profiling.region(_tag_head('head_bwd_conf', D4, H, W), nbytes, 0, logits.device):
    n = lib().mode_head_bwd_workspace_bytes(B, D4, H, W)
    ws = torch.empty(max(n // 4, 1), dtype=torch.float32, device=logits.device)
    _call('mode_head_bwd_conf', ptr(logits), ptr(pred), ptr(conf), ptr(gpred), ptr(gconf), ptr(gl), ptr(ws), B, D4, H4, W4, D, H, W, stream_of(logits))
  return gl


class HeadConfFunction(torch.autograd.Function):
  """(pred, conf) = head_fwd(logits, size, with_confidence=True) as ONE node: one head pass forward, one backward for both outputs."""

  @staticmethod
  def forward(ctx, logits, size):
    pred, conf = head_fwd(logits, size, with_confidence=True)
    ctx.save_for_backward(logits, pred, conf)
    ctx.size = tuple(size)
    return pred, conf

  @staticmethod
  @torch.autograd.function.once_differentiable  # (the kernel has no second derivative)
  def backward(ctx, gpred, gconf):
    logits, pred, conf = ctx.saved_tensors
    gpred = torch.zeros_like(pred) if gpred is None else gpred  # an output that nothing downstream used
    gconf = torch.zeros_like(conf) if gconf is None else gconf
    return head_bwd_conf(logits, pred, conf, gpred, gconf, ctx.size), None


def head_conf(logits, size):
  """logits (B, 1, D/4, H/4, W/4) -> (pred, conf) (B, 1, H, W) each, the bits of head_fwd(..., with_confidence=True), differentiable in
  the logits through BOTH outputs (mode_head_bwd_conf; models/mode_disparity.py:157-183 is differentiable in the probability volume:
  grid_sample(mode='nearest') passes the gradient to its input, round(pred) passes none)."""
  return HeadConfFunction.apply(logits, size)


# ------------------------------------------------------------------------------------ the three heads + the training loss, fused
# train_disparity.py:151-158: loss = 0.5 sl1(pred1[mask], gt[mask]) + 0.7 sl1(pred2[mask], ...) + sl1(pred3[mask], ...), smooth-L1 with
# mean reduction over the valid pixels.  As torch ops on the three (B, 1, H, W) maps that is ~25 small elementwise launches forward
# and as many backward; here the loss is two tiny launches (mode_smooth_l1_masked) and its gradient is formed inside the head's
# backward kernel from the forward's own prediction (mode_head_bwd_loss): nothing elementwise between the heads and the optimizer.
def head_loss_supported(logits, size):
  B, one, D4, H4, W4 = logits.shape
  D, H, W = size
  return (logits.is_cuda and logits.dtype == torch.float32 and one == 1 and
          lib().mode_head_loss_supported(B, D4, H4, W4, D, H, W) == 1)


class HeadLossFunction(torch.autograd.Function):
  """(loss, pred1, pred2, pred3) = f(cost1, cost2, cost3, gt, scale): pred_i = head(cost_i), loss = scale * sum_i w_i * sum over the
  pixels with a ground truth (gt == gt) of smooth_l1(pred_i - gt).  `scale` is a device scalar (1 / number of valid pixels over all
  ranks: data_parallel.global_valid_count).  The predictions are returned for inspection and carry no gradient."""

  @staticmethod
  def forward(ctx, c1, c2, c3, gt, scale, weights, size):
    costs = [c.contiguous() for c in (c1, c2, c3)]
    gt = gt.contiguous()
    require_gpu(*costs, gt, scale)
    require_f32c(*costs, gt)
    scale = scale.reshape(1).to(torch.float32)
    preds = [head_fwd(c, size) for c in costs]
    if tuple(gt.shape) != tuple(preds[0].shape):
      raise RuntimeError('head_loss: ground truth %s does not match the predictions %s' % (tuple(gt.shape), tuple(preds[0].shape)))
    n = gt.numel()
    loss = torch.empty(1, dtype=torch.float32, device=gt.device)
    with torch.cuda.device_of(gt), profiling.region('smooth_l1_masked', 4 * 4 * n, 0, gt.device):
      ws = torch.empty(max(lib().mode_smooth_l1_workspace_bytes(n) // 4, 1), dtype=torch.float32, device=gt.device)
      _call('mode_smooth_l1_masked', ptr(preds[0]), ptr(preds[1]), ptr(preds[2]), ptr(gt), float(weights[0]), float(weights[1]), float(weights[2]),
            ptr(scale), ptr(loss), ptr(ws), n, stream_of(gt))
    ctx.save_for_backward(*costs, *preds, gt, scale)
    ctx.weights, ctx.size = tuple(float(w) for w in weights), tuple(size)
    ctx.mark_non_differentiable(*preds)
    return (loss.reshape(()),) + tuple(preds)

  @staticmethod
  def backward(ctx, gloss, *unused):
    c1, c2, c3, p1, p2, p3, gt, scale = ctx.saved_tensors
    sg = (scale * gloss.reshape(1)).contiguous()  # upstream gradient of the loss folded into the scale (one 1-element launch)
    D, H, W = ctx.size
    grads = []
    for c, p, wt, need in zip((c1, c2, c3), (p1, p2, p3), ctx.weights, ctx.needs_input_grad[:3]):
      if not need:
        grads.append(None)
        continue
      B, _, D4, H4, W4 = c.shape
      gl = torch.empty_like(c)
      with torch.cuda.device_of(c), profiling.region(_tag_head('head_bwd', D4, H, W), 4 * (2 * c.numel() + 2 * p.numel()), 0, c.device):
        ws = torch.empty(max(lib().mode_head_bwd_workspace_bytes(B, D4, H, W) // 4, 1), dtype=torch.float32, device=c.device)
        _call('mode_head_bwd_loss', ptr(c), ptr(p), ptr(gt), wt, ptr(sg), ptr(gl), ptr(ws), B, D4, H4, W4, D, H, W, stream_of(c))
      grads.append(gl)
    return grads[0], grads[1], grads[2], None, None, None, None


def head_loss(costs, size, gt, scale, weights=(0.5, 0.7, 1.0)):
  """costs = (cost1, cost2, cost3) (B, 1, D/4, H/4, W/4) each -> (loss, (pred1, pred2, pred3)); head_loss_supported(costs[0], size)."""
  out = HeadLossFunction.apply(costs[0], costs[1], costs[2], gt, scale, tuple(weights), tuple(size))
  return out[0], tuple(out[1:])


# ------------------------------------------------------------------------------------ evaluation metrics and the SILog loss
# utils/evaluation.py of the reference compacts pred[mask], gt[mask] twice per metric and syncs once per metric; here a whole list of
# metrics is one pass of mode_masked_metrics over the uncompacted maps (the mask applied in the kernel) and one 8-byte-per-statistic
# copy back.  The SILog loss of train_fusion.py:82-87 is the same pass finalised on the device.
def _metrics_operands(pred, gt, mask, who):
  require_gpu(pred, gt, mask)
  for t in (pred, gt):
    if t.dtype != torch.float32:
      raise TypeError('%s: pred and gt must be float32 (got %s)' % (who, t.dtype))
  if pred.numel() != gt.numel() or (mask is not None and mask.numel() != gt.numel()):
    raise ValueError('%s: pred %s, gt %s and mask %s differ in element count' %
                     (who, tuple(pred.shape), tuple(gt.shape), None if mask is None else tuple(mask.shape)))
  if mask is not None:
    if mask.dtype != torch.bool:
      raise TypeError('%s: the mask must be torch.bool (got %s)' % (who, mask.dtype))
    mask = mask.contiguous().view(torch.uint8)
  return pred.contiguous(), gt.contiguous(), mask


def _metrics_workspace(n, device):
  return torch.empty(max(lib().mode_masked_metrics_workspace_bytes(n) // 8, 1), dtype=torch.float64, device=device)


def _metrics_params(px, d1, ratio, who):
  if max(len(px), len(d1), len(ratio)) > METRICS_MAX_THRESHOLDS:
    raise ValueError('%s: at most %d thresholds of each kind' % (who, METRICS_MAX_THRESHOLDS))
  prm = MetricsParams()
  prm.n_px, prm.n_d1, prm.n_ratio = len(px), len(d1), len(ratio)
  for k, t in enumerate(px):
    prm.px[k] = float(t)
  for k, (tp, tc) in enumerate(d1):
    prm.d1_px[k], prm.d1_pct[k] = float(tp), float(tc)
  for k, r in enumerate(ratio):
    prm.ratio[k] = float(r)
  return prm


def masked_metrics(pred, gt, mask=None, px=(), d1=(), ratio=()):
  """The statistic vector of mode_masked_metrics (include/mode_hip.h) over the elements `mask` selects (None: all) as a float64 numpy
  array of METRICS_COUNT entries (indices mode_hip.M_*): one launch pair and one small device-to-host copy.  px: thresholds of
  pixel_error_pct; d1: (th_pixel, th_pct) pairs of D1; ratio: bounds of delta_acc / threshold_acc (each rounded to fp32 as torch does)."""
  pred, gt, mask = _metrics_operands(pred, gt, mask, 'masked_metrics')
  prm = _metrics_params(px, d1, ratio, 'masked_metrics')
  n = gt.numel()
  out = torch.empty(METRICS_COUNT, dtype=torch.float64, device=gt.device)
  with torch.cuda.device_of(gt), profiling.region('masked_metrics', (8 + (1 if mask is not None else 0)) * n, 0, gt.device):
    ws = _metrics_workspace(n, gt.device)
    _call('mode_masked_metrics', ptr(pred), ptr(gt), _optr(mask), n, ctypes.byref(prm), ptr(ws), ws.numel() * 8, ptr(out), stream_of(gt))
  return out.cpu().numpy()


class SilogLossFunction(torch.autograd.Function):
  """loss = mean(l^2) - lamda mean(l)^2, l = log pred - log gt over the elements with mask, gt > 0 and pred > 0 (train_fusion.py:82-87
  on pred[mask], gt[mask]): a device scalar, NaN with a zero gradient when nothing is selected, as torch's."""

  @staticmethod
  def forward(ctx, pred, gt, mask, lamda):
    p, g, m = _metrics_operands(pred, gt, mask, 'silog_loss')
    n = g.numel()
    stats = torch.empty(METRICS_COUNT, dtype=torch.float64, device=g.device)
    loss = torch.empty(1, dtype=torch.float32, device=g.device)
    with torch.cuda.device_of(g), profiling.region('silog_loss_fwd', (8 + (1 if m is not None else 0)) * n, 0, g.device):
      ws = _metrics_workspace(n, g.device)
      _call('mode_silog_loss_fwd', ptr(p), ptr(g), _optr(m), n, float(lamda), ptr(ws), ws.numel() * 8, ptr(stats), ptr(loss), stream_of(g))
    ctx.save_for_backward(p, g, m if m is not None else torch.empty(0, dtype=torch.uint8, device=g.device), stats)
    ctx.has_mask, ctx.lamda, ctx.shape = m is not None, float(lamda), pred.shape
    return loss.reshape(())

  @staticmethod
  def backward(ctx, gloss):
    p, g, m, stats = ctx.saved_tensors
    n = g.numel()
    gl = gloss.reshape(1).to(torch.float32).contiguous()
    gp = torch.empty_like(p)
    with torch.cuda.device_of(g), profiling.region('silog_loss_bwd', (12 + (1 if ctx.has_mask else 0)) * n, 0, g.device):
      _call('mode_silog_loss_bwd', ptr(p), ptr(g), ptr(m) if ctx.has_mask else None, n, ctx.lamda, ptr(stats), ptr(gl), ptr(gp), stream_of(g))
    return gp.view(ctx.shape), None, None, None


def silog_loss(pred, gt, mask=None, lamda=0.5):
  """The fusion stage's training loss (train_fusion.py:82-87 applied at :100-111 as silog_loss(0.5, output[mask], gt[mask])) without
  the compaction: `mask` is the outer selection (gt <= maxdepth; None: every element), gt > 0 and pred > 0 are applied inside.  pred
  may be (B, 1, H, W) with gt and mask (B, H, W).  Returns a 0-d device tensor; no host synchronisation (graph-capturable)."""
  return SilogLossFunction.apply(pred, gt, mask, lamda)


# ------------------------------------------------------------------------------------ self-supervised stereo loss
# Composed from torch operators the loss is about 60 elementwise, pooling and gather launches per disparity map, with autograd's
# scatter in the backward; here it is two launches forward and one backward for all K maps (csrc/photometric.hip), bit-repeatable.
def _photometric_params(K, weights, alpha, lam, beta, mean, std, c1=1e-4, c2=9e-4):
  from dataloader.preprocess import imagenet_stats
  mean = imagenet_stats['mean'] if mean is None else mean
  std = imagenet_stats['std'] if std is None else std
  if len(mean) != 3 or len(std) != 3:
    raise ValueError('photometric_loss: mean and std have one entry per colour channel (3), got %d and %d' % (len(mean), len(std)))
  if len(weights) != K:
    raise ValueError('photometric_loss: %d disparity maps but %d weights' % (K, len(weights)))
  prm = PhotometricParams()
  prm.alpha, prm.lam, prm.beta, prm.c1, prm.c2 = float(alpha), float(lam), float(beta), float(c1), float(c2)
  for c in range(3):
    prm.mean[c], prm.std[c] = float(mean[c]), float(std[c])
  for k in range(K):
    prm.weights[k] = float(weights[k])
  return prm


def _stack_maps(disps, B, H, W, like):
  """K maps (B, 1, H, W) or (B, H, W) -> one (K, B, H, W) tensor, the layout of the entries."""
  disp = torch.empty((len(disps), B, H, W), dtype=like.dtype, device=like.device)
  for k, d in enumerate(disps):
    disp[k].copy_(d.reshape(B, H, W))
  return disp


class StereoLossFunction(torch.autograd.Function):
  """(name, own, other, mask or None, view 0 / 1, prm, disp_0 .. disp_{K-1}) -> (loss 0-d, stats (K, PHOTOMETRIC_STATS) float64): one
  forward launch pair and one backward launch for all K maps.  Gradient into the disparities only (the images are data); the statistics
  carry none.  name is the entry pair and the profiling regions: 'photometric_loss' (mode_photometric_loss_fwd / _bwd, the
  left view without a mask, which is all those entries take) or 'selfsup_view_loss' (mode_selfsup_view_loss_fwd / _bwd,
  either camera and an optional mask)."""

  @staticmethod
  def _form(name, mask, view):
    """The arguments that only the entries of DESIGN 24 take."""
    return () if name == 'photometric_loss' else (None if mask is None else ptr(mask), view)

  @staticmethod
  def forward(ctx, name, own, other, mask, view, prm, *disps):
    K = len(disps)
    B, _, H, W = own.shape
    disp = _stack_maps(disps, B, H, W, own)
    require_f32c(own, other, disp)
    stats = torch.empty((K, PHOTOMETRIC_STATS), dtype=torch.float64, device=own.device)
    loss = torch.empty(1, dtype=torch.float32, device=own.device)
    nbytes = 4 * K * (own.numel() + other.numel() + disp[0].numel()) + (0 if mask is None else mask.numel())
    with torch.cuda.device_of(own), profiling.region(name + '_fwd', nbytes, 0, own.device):
      ws = torch.empty(max(lib().mode_photometric_loss_workspace_bytes(K, B, H, W) // 8, 1), dtype=torch.float64, device=own.device)
      _call('mode_%s_fwd' % name, ptr(own), ptr(other), ptr(disp), *StereoLossFunction._form(name, mask, view), K, B, H, W,
            ctypes.byref(prm), ptr(ws), ws.numel() * 8, ptr(stats), ptr(loss), stream_of(own))
    ctx.save_for_backward(own, other, disp, stats, *(() if mask is None else (mask,)))
    ctx.name, ctx.view, ctx.prm, ctx.shapes = name, view, prm, [d.shape for d in disps]
    ctx.mark_non_differentiable(stats)
    return loss.reshape(()), stats

  @staticmethod
  def backward(ctx, gloss, _gstats):
    own, other, disp, stats = ctx.saved_tensors[:4]
    mask = ctx.saved_tensors[4] if len(ctx.saved_tensors) > 4 else None
    K, B, H, W = disp.shape
    gl = gloss.reshape(1).to(torch.float32).contiguous()
    gdisp = torch.empty_like(disp)
    nbytes = 4 * K * (own.numel() + other.numel() + 2 * disp[0].numel()) + (0 if mask is None else mask.numel())
    with torch.cuda.device_of(own), profiling.region(ctx.name + '_bwd', nbytes, 0, own.device):
      _call('mode_%s_bwd' % ctx.name, ptr(own), ptr(other), ptr(disp), *StereoLossFunction._form(ctx.name, mask, ctx.view), K, B, H, W,
            ctypes.byref(ctx.prm), ptr(stats), ptr(gl), ptr(gdisp), stream_of(own))
    return (None,) * 6 + tuple(gdisp[k].view(shape) for k, shape in enumerate(ctx.shapes))


class PhotometricLossFunction:
  """StereoLossFunction through the entries of DESIGN 22: apply(left, right, prm, disp_0 .. disp_{K-1})."""
  apply = staticmethod(lambda left, right, prm, *disps: StereoLossFunction.apply('photometric_loss', left, right, None, 0, prm, *disps))


class ViewLossFunction:
  """StereoLossFunction through the entries of DESIGN 24: apply(own, other, mask or None, view 0 / 1, prm, disp_0 .. disp_{K-1})."""
  apply = staticmethod(lambda *args: StereoLossFunction.apply('selfsup_view_loss', *args))


def photometric_loss(left, right, disps, weights, alpha=0.85, lam=0.1, beta=1.0, mean=None, std=None, return_stats=False, view='left',
                     masks=None):
  """The self-supervised loss of a rectified Cassini stereo pair (include/mode_hip.h has the definition): the right image
  warped to the left view by each disparity map, SSIM + L1 over 3x3 windows whose rows wrap along H, plus lam x an edge-aware smoothness
  term, summed over the maps with `weights`.  left, right (B, 3, H, W) as the model takes them (normalised with mean / std, default
  dataloader.preprocess.imagenet_stats); disps: 1 .. 4 tensors (B, 1, H, W) or (B, H, W), e.g. the three training outputs.  Returns a
  0-d device tensor with autograd into every map (not into the images); with return_stats also a (K, 3) float64 device tensor
  [N_valid, photo, smooth] per map.  No host synchronisation; the counts stay on the device.

  view, masks: with view='right' the first image is the RIGHT camera's (it supplies L and the smoothness edges), the second the
  left camera's, the maps are right-view disparities and the warp is x = w + d.  masks: a (K, B, H, W) uint8 or bool device tensor, e.g.
  lr_consistency's masks[0] (left) or masks[1] (right): a pixel whose byte is zero is invalid; the mask carries no gradient.  The defaults
  take the entries of DESIGN 22; either option goes through mode_selfsup_view_loss_fwd / _bwd."""
  disps = list(disps)
  if view not in ('left', 'right'):
    raise ValueError("photometric_loss: view must be 'left' or 'right', not %r" % (view,))
  require_gpu(left, right, masks, *disps)
  K = len(disps)
  if not 1 <= K <= PHOTOMETRIC_MAX_MAPS:
    raise ValueError('photometric_loss: %d disparity maps (1 .. %d)' % (K, PHOTOMETRIC_MAX_MAPS))
  if left.dim() != 4 or left.shape[1] != 3 or right.shape != left.shape:
    raise ValueError('photometric_loss: left and right must be (B, 3, H, W), got %s and %s' % (tuple(left.shape), tuple(right.shape)))
  B, _, H, W = left.shape
  for d in disps:
    if tuple(d.shape) not in ((B, 1, H, W), (B, H, W)):
      raise ValueError('photometric_loss: a disparity map of shape %s for images %s' % (tuple(d.shape), tuple(left.shape)))
  prm = _photometric_params(K, weights, alpha, lam, beta, mean, std)
  if masks is not None:
    if tuple(masks.shape) != (K, B, H, W) or masks.dtype not in (torch.uint8, torch.bool):
      raise ValueError('photometric_loss: masks must be a (K, B, H, W) = %s uint8 or bool tensor, got %s %s' % (
          (K, B, H, W), tuple(masks.shape), masks.dtype))
    masks = masks.detach().contiguous()
    masks = masks.view(torch.uint8) if masks.dtype == torch.bool else masks
  name = 'photometric_loss' if view == 'left' and masks is None else 'selfsup_view_loss'
  loss, stats = StereoLossFunction.apply(name, left.contiguous(), right.contiguous(), masks, 0 if view == 'left' else 1, prm, *disps)
  if not return_stats:
    return loss
  n = stats[:, 0]
  photo = stats[:, 1] / n.clamp(min=1)
  smooth = stats[:, 2] / (B * H * (W - 1)) + stats[:, 3] / (B * H * W)
  return loss, torch.stack([n, photo, smooth], 1)


# ------------------------------------------------------------------------------------ left-right consistency
# The remedy for occlusion in a photometric loss: both views' disparities, their disagreement as a loss, and the pixels where they
# disagree kept out of the photometric term.  Composed from torch operators the gradient into the sampled map is a scatter with atomics;
# csrc/lr_consistency.hip gathers it over a bounded window, bit-repeatable: two launches forward, one backward, for both views and K maps.
class LrConsistencyFunction(torch.autograd.Function):
  """(prm, want_masks, K, dl_0 .. dl_{K-1}, dr_0 .. dr_{K-1}) -> (loss 0-d, stats (2, K, LR_STATS) float64, masks (2, K, B, H, W) uint8 or
  an empty tensor).  Gradients into every map of both lists; the statistics and the masks carry none."""

  @staticmethod
  def forward(ctx, prm, want_masks, K, *maps):
    first = maps[0]
    B, H, W = first.shape[0], first.shape[-2], first.shape[-1]
    dl, dr = _stack_maps(maps[:K], B, H, W, first), _stack_maps(maps[K:], B, H, W, first)
    require_f32c(dl, dr)
    dev = first.device
    stats = torch.empty((2, K, LR_STATS), dtype=torch.float64, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    masks = torch.empty((2, K, B, H, W) if want_masks else (0,), dtype=torch.uint8, device=dev)
    nbytes = 8 * dl.numel() + masks.numel()
    with torch.cuda.device_of(first), profiling.region('lr_consistency_fwd', nbytes, 0, dev):
      ws = torch.empty(max(lib().mode_lr_consistency_workspace_bytes(K, B, H, W) // 8, 1), dtype=torch.float64, device=dev)
      _call('mode_lr_consistency_fwd', ptr(dl), ptr(dr), K, B, H, W, ctypes.byref(prm), ptr(ws), ws.numel() * 8,
            ptr(masks) if want_masks else None, ptr(stats), ptr(loss), stream_of(first))
    ctx.save_for_backward(dl, dr, stats)
    ctx.prm, ctx.shapes = prm, [d.shape for d in maps]
    ctx.mark_non_differentiable(stats, masks)
    return loss.reshape(()), stats, masks

  @staticmethod
  def backward(ctx, gloss, _gstats, _gmasks):
    dl, dr, stats = ctx.saved_tensors
    K, B, H, W = dl.shape
    gl = gloss.reshape(1).to(torch.float32).contiguous()
    gdl, gdr = torch.empty_like(dl), torch.empty_like(dr)
    with torch.cuda.device_of(dl), profiling.region('lr_consistency_bwd', 16 * dl.numel(), 0, dl.device):
      _call('mode_lr_consistency_bwd', ptr(dl), ptr(dr), K, B, H, W, ctypes.byref(ctx.prm), ptr(stats), ptr(gl), ptr(gdl), ptr(gdr),
            stream_of(dl))
    grads = [gdl[k] for k in range(K)] + [gdr[k] for k in range(K)]
    return (None, None, None) + tuple(g.view(shape) for g, shape in zip(grads, ctx.shapes))


def lr_consistency(disps_l, disps_r, weights, tau=1.0, dmax=None, return_masks=False, return_stats=False):
  """Left-right consistency of a Cassini pair's disparity maps (include/mode_hip_selfsup.h has the definition).  disps_l,
  disps_r: K = 1 .. 4 tensors each, (B, 1, H, W) or (B, H, W): left pixel (h, w) matches right pixel (h, w - dl), right pixel (h, w)
  matches left pixel (h, w + dr).  Per view and map the mean over the valid pixels of |own - other(x)|, x = w -/+ own (valid: own finite
  and in [0, dmax], x inside the row, both samples finite), summed over views and maps with `weights`.  dmax (required, e.g. the
  model's maxdisp) bounds the disparities that take part, and with them the window the backward gathers over.  Returns a 0-d device
  tensor with autograd into every map of both lists; with return_masks also the visibility masks (2, K, B, H, W) uint8 (left, right;
  1 = valid and |own - other(x)| <= tau; no gradient), which HF.photometric_loss(..., masks=masks[v]) takes; with return_stats also a
  (2, K, 3) float64 device tensor [N_valid, lr, N_visible].  Order of the extras: masks, stats.  No host synchronisation."""
  disps_l, disps_r = list(disps_l), list(disps_r)
  require_gpu(*(disps_l + disps_r))
  K = len(disps_l)
  if not 1 <= K <= PHOTOMETRIC_MAX_MAPS or len(disps_r) != K:
    raise ValueError('lr_consistency: %d left and %d right disparity maps (1 .. %d of each, as many left as right)' % (
        K, len(disps_r), PHOTOMETRIC_MAX_MAPS))
  if len(weights) != K:
    raise ValueError('lr_consistency: %d disparity maps per view but %d weights' % (K, len(weights)))
  if dmax is None:
    raise ValueError('lr_consistency: dmax is required (the largest disparity that takes part, e.g. the maxdisp of the model)')
  first = disps_l[0]
  if first.dim() not in (3, 4) or (first.dim() == 4 and first.shape[1] != 1):
    raise ValueError('lr_consistency: a disparity map is (B, 1, H, W) or (B, H, W), got %s' % (tuple(first.shape),))
  B, H, W = first.shape[0], first.shape[-2], first.shape[-1]
  for d in disps_l + disps_r:
    if tuple(d.shape) not in ((B, 1, H, W), (B, H, W)):
      raise ValueError('lr_consistency: a disparity map of shape %s among maps of %s' % (tuple(d.shape), (B, H, W)))
  prm = LrParams()
  prm.tau, prm.dmax = float(tau), float(dmax)
  for k in range(K):
    prm.weights[k] = float(weights[k])
  loss, stats, masks = LrConsistencyFunction.apply(prm, bool(return_masks), K, *(disps_l + disps_r))
  out = (loss,)
  if return_masks:
    out += (masks,)
  if return_stats:
    out += (torch.stack([stats[..., 0], stats[..., 1] / stats[..., 0].clamp(min=1), stats[..., 2]], -1),)
  return out[0] if len(out) == 1 else out


# ------------------------------------------------------------------------------------ multi-view reprojection loss
# The self-supervised loss of the fused depth: every pixel lifted by its depth, projected into S other panoramas of known pose and
# compared there, the per-window minimum over the views.  Composed from torch operators it is some 70 launches per source and a
# scatter with atomics in the backward; csrc/mv_photometric.hip runs the source loop inside one kernel per pass, bit-repeatable.
class MvPhotometricLossFunction(torch.autograd.Function):
  """(ref, src, depth, poses (S, 12) float64 numpy, prm) -> (loss 0-d, stats (MVP_STATS,) float64, win (F, H, W) uint8).  Gradient
  into depth only (the images are data); the statistics and the winners carry none."""

  @staticmethod
  def forward(ctx, ref, src, depth, poses, prm, masks=None):
    F, S, _, H, W = src.shape
    d = depth.reshape(F, H, W).contiguous()
    require_f32c(ref, src, d)
    dev = ref.device
    stats = torch.empty(MVP_STATS, dtype=torch.float64, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    win = torch.empty((F, H, W), dtype=torch.uint8, device=dev)
    pp = poses.ctypes.data_as(ctypes.c_void_p)
    nbytes = 4 * (ref.numel() + src.numel() + d.numel()) + win.numel()
    if masks is None:
      with torch.cuda.device_of(ref), profiling.region('mv_photometric_loss_fwd', nbytes, 0, dev):
        ws = torch.empty(max(lib().mode_mvphoto_workspace_bytes(S, F, H, W) // 8, 1), dtype=torch.float64, device=dev)
        _call('mode_mvphoto_loss_fwd', ptr(ref), ptr(src), ptr(d), pp, S, F, H, W, ctypes.byref(prm), ptr(ws), ws.numel() * 8, ptr(win),
              ptr(stats), ptr(loss), stream_of(ref))
    else:  # the same loss over the pixels that each source sees; win and stats then serve the two backward entries as they are
      with torch.cuda.device_of(ref), profiling.region('mv_photometric_loss_fwd', nbytes + masks.numel(), 0, dev):
        ws = torch.empty(max(lib().mode_mvphoto_workspace_bytes(S, F, H, W) // 8, 1), dtype=torch.float64, device=dev)
        _call('mode_mvphoto_loss_fwd_masked', ptr(ref), ptr(src), ptr(d), pp, S, F, H, W, ctypes.byref(prm), ptr(ws), ws.numel() * 8,
              ptr(masks), ptr(win), ptr(stats), ptr(loss), stream_of(ref))
    ctx.save_for_backward(ref, src, d, win, stats)
    ctx.prm, ctx.poses, ctx.shape, ctx.extra = prm, poses, depth.shape, () if masks is None else (None,)
    ctx.mark_non_differentiable(stats, win)
    return loss.reshape(()), stats, win

  @staticmethod
  def backward(ctx, gloss, _gstats, _gwin):
    ref, src, d, win, stats = ctx.saved_tensors
    F, S, _, H, W = src.shape
    gl = gloss.reshape(1).to(torch.float32).contiguous()
    gdepth = torch.empty_like(d)
    nbytes = 4 * (ref.numel() + src.numel() + 2 * d.numel()) + win.numel()
    with torch.cuda.device_of(ref), profiling.region('mv_photometric_loss_bwd', nbytes, 0, ref.device):
      _call('mode_mvphoto_loss_bwd', ptr(ref), ptr(src), ptr(d), ctx.poses.ctypes.data_as(ctypes.c_void_p), S, F, H, W, ctypes.byref(ctx.prm),
            ptr(win), ptr(stats), ptr(gl), ptr(gdepth), stream_of(ref))
    return (None, None, gdepth.view(ctx.shape), None, None) + ctx.extra


class MvPhotometricPoseLossFunction(torch.autograd.Function):
  """MvPhotometricLossFunction with the poses as an input of the graph: poses is a float64 CPU tensor (S, 12) or (S, 3, 4).
  The forward is that function's; the backward runs mode_mvphoto_loss_bwd if the depth needs a gradient and mode_mvpose_grad
  (csrc/mv_pose_grad.hip) if the poses do, and returns the latter on the host in the input's shape: one device-to-host copy, so this
  backward synchronises."""

  @staticmethod
  def forward(ctx, ref, src, depth, poses, prm, masks=None):
    import numpy as np
    ctx.pose_shape = poses.shape
    return MvPhotometricLossFunction.forward(ctx, ref, src, depth, np.ascontiguousarray(poses.detach().numpy().reshape(-1, 12)), prm, masks)

  @staticmethod
  def backward(ctx, gloss, _gstats, _gwin):
    gdepth = MvPhotometricLossFunction.backward(ctx, gloss, None, None)[2] if ctx.needs_input_grad[2] else None
    gposes = None
    if ctx.needs_input_grad[3]:
      ref, src, d, win, stats = ctx.saved_tensors
      F, S, _, H, W = src.shape
      dev = ref.device
      gl = gloss.reshape(1).to(torch.float32).contiguous()
      out = torch.empty((S, 12), dtype=torch.float64, device=dev)
      nbytes = 4 * (ref.numel() + src.numel() + d.numel()) + win.numel()
      with torch.cuda.device_of(ref), profiling.region('mv_pose_grad', nbytes, 0, dev):
        ws = torch.empty(max(lib().mode_mvpose_workspace_bytes(S, F, H, W) // 8, 1), dtype=torch.float64, device=dev)
        _call('mode_mvpose_grad', ptr(ref), ptr(src), ptr(d), ctx.poses.ctypes.data_as(ctypes.c_void_p), S, F, H, W, ctypes.byref(ctx.prm),
              ptr(win), ptr(stats), ptr(gl), ptr(ws), ws.numel() * 8, ptr(out), stream_of(ref))
      gposes = out.cpu().view(ctx.pose_shape)
    return (None, None, gdepth, gposes, None) + ctx.extra


def mv_photometric_loss(ref, src, depth, poses, alpha=0.85, lam=0.1, beta=1.0, mean=None, std=None, return_stats=False, return_win=False,
                        masks=None):
  """The self-supervised loss of a depth map against other panoramas of known pose (include/mode_hip_mvphoto.h has the
  definition): ref (F, 3, H, W) is the Cassini panorama the depth map belongs to, src (F, S, 3, H, W) are S = 1 .. 8 other panoramas of
  the same scene, both normalised as the model takes them (mean / std, default dataloader.preprocess.imagenet_stats); depth (F, 1, H, W)
  or (F, H, W); poses (S, 12) or (S, 3, 4) float64 on the host (numpy, a CPU tensor or nested lists): [A | o] per source, X_s = A X + o
  (utils.rig.CameraRig.panorama_poses()[sources]).  Every pixel is lifted by its depth, projected into each source and sampled there;
  SSIM + L1 over 3x3 windows whose rows wrap along H, the minimum over the sources per window, plus lam x an edge-aware smoothness term
  on log depth.  Returns a 0-d device tensor with autograd into depth (not into the images); with return_stats also a (3 + S,) float64
  device tensor [N, photo, smooth, wins of source 0 .. S - 1]; with return_win also the (F, H, W) uint8 map of the winning source per
  window (255: none).  Order of the extras: stats, win.  No host synchronisation.

  Self-calibration (include/mode_hip_mvpose.h): when poses is a torch.Tensor with requires_grad -- float64 on the CPU,
  (S, 12) or (S, 3, 4), e.g. utils.rig_refine.RigRefinement(rig)()[sources] -- the gradient flows into it as well: (S, 12) holds
  d loss / d A in the first three columns of each 3 x 4 table and d loss / d o in the fourth.  That gradient comes back to the host,
  one device-to-host copy, so backward() then synchronises; every other form of poses runs exactly as before.  The gradient is
  one-sided where v is an integer (exactly rectified poses: the right camera of the reference's own pair), and a source that wins
  no window gets an exactly zero row: calibrate a source at a time, or only sources that are comparably off.

  Visibility (include/mode_hip_mvvis.h): masks is a (F, S, H, W) uint8 device tensor, e.g. HF.mv_visibility(depth.detach(),
  poses); a pixel then counts as valid for source s only where masks[f, s, h, w] != 0, so a source wins a window only if it sees all
  nine of its pixels.  The masks are constants of the gradient; the gradients to the depth and to a pose tensor run as without."""
  import numpy as np
  require_gpu(ref, src, depth)
  if ref.dim() != 4 or ref.shape[1] != 3:
    raise ValueError('mv_photometric_loss: ref must be (F, 3, H, W), got %s' % (tuple(ref.shape),))
  F, _, H, W = ref.shape
  if src.dim() != 5 or tuple(src.shape[:1] + src.shape[2:]) != (F, 3, H, W):
    raise ValueError('mv_photometric_loss: src must be (F, S, 3, H, W) = (%d, S, 3, %d, %d), got %s' % (F, H, W, tuple(src.shape)))
  S = src.shape[1]
  if not 1 <= S <= MVP_MAX_SOURCES:
    raise ValueError('mv_photometric_loss: %d source views (1 .. %d)' % (S, MVP_MAX_SOURCES))
  if tuple(depth.shape) not in ((F, 1, H, W), (F, H, W)):
    raise ValueError('mv_photometric_loss: a depth map of shape %s for images %s' % (tuple(depth.shape), tuple(ref.shape)))
  learned = isinstance(poses, torch.Tensor) and poses.requires_grad
  if learned:
    if poses.is_cuda or poses.dtype != torch.float64 or tuple(poses.shape) not in ((S, 12), (S, 3, 4)):
      raise ValueError('mv_photometric_loss: poses that require a gradient must be float64 on the CPU, (S, 12) or (S, 3, 4) with S = %d, '
                       'got %s %s on %s' % (S, poses.dtype, tuple(poses.shape), poses.device))
  else:
    if isinstance(poses, torch.Tensor):
      poses = poses.detach().cpu().numpy()
    poses = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 12))
    if poses.shape[0] != S:
      raise ValueError('mv_photometric_loss: %d poses for %d source views' % (poses.shape[0], S))
  prm = _photometric_params(0, (), alpha, lam, beta, mean, std)
  fn = MvPhotometricPoseLossFunction if learned else MvPhotometricLossFunction
  if masks is None:
    loss, stats, win = fn.apply(ref.contiguous(), src.contiguous(), depth, poses, prm)
  else:
    require_gpu(masks)
    if masks.dtype != torch.uint8 or tuple(masks.shape) != (F, S, H, W):
      raise ValueError('mv_photometric_loss: masks must be a (F, S, H, W) = %s uint8 tensor (HF.mv_visibility), got %s %s' % (
          (F, S, H, W), masks.dtype, tuple(masks.shape)))
    loss, stats, win = fn.apply(ref.contiguous(), src.contiguous(), depth, poses, prm, masks.contiguous())
  out = (loss,)
  if return_stats:
    smooth = stats[2] / (F * H * (W - 1)) + stats[3] / (F * H * W)
    out += (torch.cat([torch.stack([stats[0], stats[1] / stats[0].clamp(min=1), smooth]), stats[MVP_WINS:MVP_WINS + S]]),)
  if return_win:
    out += (win,)
  return out[0] if len(out) == 1 else out


# ------------------------------------------------------------------------------------ visibility of the fused depth
# The per-window minimum above chooses among whatever the sources show; a source that looks at an occluder still offers its colour.
# The fused depth forward-projected into a source is a depth map of that source (a z-buffer of 64-bit integer minima, as the hand-off's),
# and a pixel farther from the source's centre than what its landing place holds is hidden there.  Three launches for any F and S.
def mv_visibility(depth, poses, tol=0.05, radius=0, return_zbuf=False):
  """Which pixels of a depth map each of S source panoramas sees (include/mode_hip_mvvis.h has the definition): depth
  (F, 1, H, W) or (F, H, W) fp32 on the device, poses in every form HF.mv_photometric_loss takes -- (S, 12) or (S, 3, 4) float64 on the
  host as numpy, a tensor (one that requires a gradient gives its detached values: the masks are constants) or nested lists.  A pixel
  is visible to source s iff it is valid for s and its range rho to that source's centre is at most (1 + tol) times the smallest rho
  that lands on the same source pixel (radius = 0) or on its 3 x 3 neighbourhood (radius = 1: closes the holes of a magnified occluder,
  and marks slanted surfaces hidden).  Returns vis (F, S, H, W) uint8, 0 or 1, for HF.mv_photometric_loss(masks=); with return_zbuf
  also zbuf (F, S, H, W) fp32: the range map of every source view rendered from the depth, +inf where nothing lands.  No autograd,
  no host synchronisation."""
  import math

  import numpy as np
  require_gpu(depth)
  if depth.dim() not in (3, 4) or (depth.dim() == 4 and depth.shape[1] != 1):
    raise ValueError('mv_visibility: a depth map is (F, 1, H, W) or (F, H, W), got %s' % (tuple(depth.shape),))
  F, H, W = depth.shape[0], depth.shape[-2], depth.shape[-1]
  if isinstance(poses, torch.Tensor):
    poses = poses.detach().cpu().numpy()
  poses = np.asarray(poses, dtype=np.float64)
  if poses.ndim not in (2, 3) or poses.size % 12 or tuple(poses.shape[1:]) not in ((12,), (3, 4)):
    raise ValueError('mv_visibility: poses must be (S, 12) or (S, 3, 4), got %s' % (tuple(poses.shape),))
  poses = np.ascontiguousarray(poses.reshape(-1, 12))
  S = poses.shape[0]
  if not 1 <= S <= MVP_MAX_SOURCES:
    raise ValueError('mv_visibility: %d source views (1 .. %d)' % (S, MVP_MAX_SOURCES))
  tol = float(tol)
  if not (math.isfinite(tol) and tol >= 0):
    raise ValueError('mv_visibility: tol = %r must be finite and >= 0' % (tol,))
  if radius not in (0, 1):
    raise ValueError('mv_visibility: radius = %r (0 or 1)' % (radius,))
  d = depth.detach().reshape(F, H, W).contiguous()
  require_f32c(d)
  dev = d.device
  vis = torch.empty((F, S, H, W), dtype=torch.uint8, device=dev)
  zbuf = torch.empty((F, S, H, W), dtype=torch.float32, device=dev) if return_zbuf else None
  n = vis.numel()
  with torch.cuda.device_of(d), profiling.region('mv_visibility', 4 * d.numel() + (2 * 20 + 8 + 1 + (4 if return_zbuf else 0)) * n, 0, dev):
    ws = torch.empty(max(lib().mode_mvvis_workspace_bytes(S, F, H, W) // 8, 1), dtype=torch.float64, device=dev)
    _call('mode_mv_visibility', ptr(d), poses.ctypes.data_as(ctypes.c_void_p), S, F, H, W, tol, int(radius), ptr(ws), ws.numel() * 8, ptr(vis),
          _optr(zbuf), stream_of(d))
  return (vis, zbuf) if return_zbuf else vis


# ------------------------------------------------------------------------------------ novel-view rendering
# What the fused depth map means, shown: the reference panorama lifted by it and splatted into other views.  The z-buffer is the
# visibility's; every target pixel names the reference pixel it shows, and takes its colour or the bilinear value around the point
# where its own ray at that range falls back into the reference.  Four launches for any F, T <= 8 and C.
_MVR_MODES = {'splat': MVR_SPLAT, 'resample': MVR_RESAMPLE}


def mv_render(image, depth, poses, tol=0.05, fill=1, mode='resample', return_range=False, return_hit=False, return_index=False):
  """A panorama seen from T other poses through its depth map (include/mode_hip_mvrender.h has the definition): image
  (F, C, H, W) fp32 on the device with C = 1 .. 4, taken as it is (normalised or not: values are copied or interpolated); depth
  (F, 1, H, W) or (F, H, W) and poses in every form HF.mv_visibility takes, (T, 12) or (T, 3, 4) [A | o] with X_t = A X + o
  (utils.rig.view_pose(centre, rotation) builds one).  Every pixel is lifted by its depth and lands in each target view; the nearest
  one owns a target pixel.  fill = 1 closes holes from the 3 x 3 neighbourhood and replaces a surface that is more than (1 + tol)
  times farther than the nearest neighbour's (seen through the cracks of a magnified near surface); fill = 0 leaves holes.
  mode = 'splat' copies the owning pixel's colour; 'resample' samples the image bilinearly where the target pixel's own ray, at the
  range found, falls back into the reference (sharper; the pixels beyond the reference's poles take the splat's value).  Returns out
  (F, T, C, H, W) fp32, 0 where nothing is seen; the extras follow in the order range (F, T, H, W) fp32, +inf where nothing is seen;
  hit (F, T, H, W) uint8: 0 nothing, 1 direct, 2 filled, plus 4 where resampled; index (F, T, H, W) int32: the reference pixel
  h W + w shown, -1 for none.  T > 8 runs in chunks of 8.  No autograd (the inputs are detached), no host synchronisation."""
  import math

  import numpy as np
  require_gpu(image, depth)
  if image.dim() != 4 or not 1 <= image.shape[1] <= MVR_MAX_CHANNELS:
    raise ValueError('mv_render: image must be (F, C, H, W) with C = 1 .. %d, got %s' % (MVR_MAX_CHANNELS, tuple(image.shape)))
  F, C, H, W = image.shape
  if tuple(depth.shape) not in ((F, 1, H, W), (F, H, W)):
    raise ValueError('mv_render: a depth map of shape %s for an image %s' % (tuple(depth.shape), tuple(image.shape)))
  if isinstance(poses, torch.Tensor):
    poses = poses.detach().cpu().numpy()
  poses = np.asarray(poses, dtype=np.float64)
  if poses.ndim not in (2, 3) or poses.size % 12 or tuple(poses.shape[1:]) not in ((12,), (3, 4)):
    raise ValueError('mv_render: poses must be (T, 12) or (T, 3, 4), got %s' % (tuple(poses.shape),))
  poses = np.ascontiguousarray(poses.reshape(-1, 12))
  T = poses.shape[0]
  if T < 1:
    raise ValueError('mv_render: no target view')
  tol = float(tol)
  if not (math.isfinite(tol) and tol >= 0):
    raise ValueError('mv_render: tol = %r must be finite and >= 0' % (tol,))
  if fill not in (0, 1):
    raise ValueError('mv_render: fill = %r (0 or 1)' % (fill,))
  if mode not in _MVR_MODES:
    raise ValueError("mv_render: mode = %r ('splat' or 'resample')" % (mode,))
  img = image.detach().contiguous()
  d = depth.detach().reshape(F, H, W).contiguous()
  require_f32c(img, d)
  dev = d.device
  out = torch.empty((F, T, C, H, W), dtype=torch.float32, device=dev)
  hit = torch.empty((F, T, H, W), dtype=torch.uint8, device=dev)
  rng = torch.empty((F, T, H, W), dtype=torch.float32, device=dev) if return_range else None
  index = torch.empty((F, T, H, W), dtype=torch.int32, device=dev) if return_index else None
  per_pair = 2 * 20 + 2 * 12 + 8 + 1 + 8 * C + (4 if return_range else 0) + (4 if return_index else 0)
  with torch.cuda.device_of(d), profiling.region('mv_render', 4 * d.numel() + per_pair * hit.numel(), 0, dev):
    for t0 in range(0, T, MVP_MAX_SOURCES):  # a call takes up to 8 views
      n = min(MVP_MAX_SOURCES, T - t0)
      whole = n == T
      o, h = (out, hit) if whole else (out.new_empty((F, n, C, H, W)), hit.new_empty((F, n, H, W)))
      r = rng if whole or rng is None else rng.new_empty((F, n, H, W))
      i = index if whole or index is None else index.new_empty((F, n, H, W))
      ws = torch.empty(max(lib().mode_mvrender_workspace_bytes(n, F, H, W) // 8, 1), dtype=torch.float64, device=dev)
      _call('mode_mv_render', ptr(img), ptr(d), poses[t0:t0 + n].ctypes.data_as(ctypes.c_void_p), n, F, C, H, W, tol, int(fill), _MVR_MODES[mode],
            ptr(ws), ws.numel() * 8, ptr(o), ptr(h), _optr(r), _optr(i), stream_of(d))
      if not whole:
        for whole_t, part_t in ((out, o), (hit, h), (rng, r), (index, i)):
          if whole_t is not None:
            whole_t[:, t0:t0 + n] = part_t
  extras = tuple(x for x, want in ((rng, return_range), (hit, return_hit), (index, return_index)) if want)
  return (out,) + extras if extras else out


# ------------------------------------------------------------------------------------ scoring in the ERP domain
# test_fusion.py:76-100 per batch: an optional x2 bicubic upsampling of the prediction, cassini2Equirec of prediction and ground truth,
# the gt <= maxdepth selection and eight metrics -- here one upsampling launch and one fused launch pair for any number of frames.
def erp_depth_metrics(pred, gt, grid, maxdepth, ratio=(), px=(), d1=(), return_erp=False):
  """pred, gt (F, H, W) Cassini maps (H == 2 W), grid (1, W, H, 2) or (W, H, 2): the sample points of cassini2Equirec
  (utils.geometry._c2e_grid) -> the (F, METRICS_COUNT) float64 DEVICE tensor of mode_erp_depth_metrics: row f is the statistic
  vector of masked_metrics over frame f's ERP pixels with gt_erp <= maxdepth, bit for bit.  No host synchronisation
  (graph-capturable).  return_erp: also the resampled (F, W, H) maps, (stats, pred_erp, gt_erp)."""
  require_gpu(pred, gt, grid)
  require_f32c(pred, gt, grid)
  if pred.dim() != 3 or pred.shape != gt.shape:
    raise ValueError('erp_depth_metrics: pred %s and gt %s must both be (F, H, W)' % (tuple(pred.shape), tuple(gt.shape)))
  F, H, W = pred.shape
  if H != 2 * W or H == 0:
    raise ValueError('erp_depth_metrics: a Cassini frame is H = 2 W, got %d x %d' % (H, W))
  if grid.numel() != 2 * H * W or tuple(grid.shape[-3:]) != (W, H, 2):
    raise ValueError('erp_depth_metrics: grid %s is not (W, H, 2) = (%d, %d, 2)' % (tuple(grid.shape), W, H))
  prm = _metrics_params(px, d1, ratio, 'erp_depth_metrics')
  out = torch.empty((F, METRICS_COUNT), dtype=torch.float64, device=gt.device)
  pe = torch.empty((F, W, H), dtype=torch.float32, device=gt.device) if return_erp else None
  ge = torch.empty((F, W, H), dtype=torch.float32, device=gt.device) if return_erp else None
  nbytes = (16 + (8 if return_erp else 0)) * F * H * W
  with torch.cuda.device_of(gt), profiling.region('erp_depth_metrics', nbytes, 0, gt.device):
    ws = torch.empty(max(lib().mode_erp_depth_metrics_workspace_bytes(F, H, W) // 8, 1), dtype=torch.float64, device=gt.device)
    _call('mode_erp_depth_metrics', ptr(pred), ptr(gt), ptr(grid), F, H, W, float(maxdepth), ctypes.byref(prm), ptr(ws), ws.numel() * 8, ptr(out),
          _optr(pe), _optr(ge), stream_of(gt))
  return (out, pe, ge) if return_erp else out


def bicubic_up2(x):
  """(N, C, H, W) -> (N, C, 2H, 2W) as F.interpolate(x, scale_factor=[2, 2], mode='bicubic', align_corners=True) (test_fusion.py:82)
  on mode_bicubic_up2."""
  require_gpu(x)
  require_f32c(x)
  if x.dim() != 4 or 0 in x.shape[1:]:
    raise ValueError('bicubic_up2: expected a non-empty (N, C, H, W) tensor, got %s' % (tuple(x.shape),))
  N, C, H, W = x.shape
  y = torch.empty((N, C, 2 * H, 2 * W), dtype=x.dtype, device=x.device)
  with torch.cuda.device_of(x), profiling.region('bicubic_up2', 4 * 5 * x.numel(), 2 * 20 * y.numel(), x.device):
    _call('mode_bicubic_up2', ptr(x), ptr(y), N, C, H, W, stream_of(x))
  return y


# ------------------------------------------------------------------------------------ 8-bit ingest of whole frames
def require_u8_frames(frames_u8, who):
  """(F, 12, H, W, 3) contiguous uint8 on a GPU, or TypeError / NotImplementedError / ValueError."""
  if not torch.is_tensor(frames_u8) or frames_u8.dtype != torch.uint8:
    raise TypeError('%s: frames must be a uint8 tensor (got %s)' % (who, getattr(frames_u8, 'dtype', type(frames_u8))))
  require_gpu(frames_u8)
  if not frames_u8.is_contiguous():
    raise TypeError('%s: frames must be contiguous' % who)
  if frames_u8.dim() != 5 or frames_u8.shape[1] != 12 or frames_u8.shape[4] != 3:
    raise ValueError('%s: frames must be (F, 12, H, W, 3), got %s' % (who, tuple(frames_u8.shape)))


def frames_u8_ingest(frames_u8, lut, want_rgb=True):
  """(F, 12, H, W, 3) uint8 frames and the (256, 3) normalisation table -> (left (6F, 3, H, W), right (6F, 3, H, W), rgb (F, 12, H, W)
  or None) on mode_frames_u8_ingest (dataloader.gpu_ingest.frames_u8_gpu builds the table)."""
  require_u8_frames(frames_u8, 'frames_u8_ingest')
  require_gpu(lut)
  require_f32c(lut)
  F, _, H, W, _ = frames_u8.shape
  if tuple(lut.shape) != (256, 3) or (H * W) % 4 or H * W == 0:
    raise ValueError('frames_u8_ingest: lut %s must be (256, 3) and H W = %d x %d a positive multiple of 4' % (tuple(lut.shape), H, W))
  dev = frames_u8.device
  left = torch.empty((6 * F, 3, H, W), dtype=torch.float32, device=dev)
  right = torch.empty((6 * F, 3, H, W), dtype=torch.float32, device=dev)
  rgb = torch.empty((F, 12, H, W), dtype=torch.float32, device=dev) if want_rgb else None
  nbytes = frames_u8.numel() * 5 + (0 if rgb is None else 4 * rgb.numel())
  with torch.cuda.device_of(frames_u8), profiling.region('frames_u8_ingest', nbytes, 0, dev):
    _call('mode_frames_u8_ingest', ptr(frames_u8), ptr(lut), F, H, W, ptr(left), ptr(right), _optr(rgb), stream_of(frames_u8))
  return left, right, rgb


def images_u8_augment(images_u8, ops, coef, dst=None, out=None, return_means=False):
  """(N, H, W, 3) uint8 images -> the colour-augmented, ImageNet-normalised planes (N, 3, H, W) on mode_images_u8_augment (the reference's
  inception_color_preproccess, dataloader/preprocess.py:33-46, 78-95; the contract is in include/mode_hip.h).  ops (N, 3) int32: the
  operations of every image in order (0 brightness, 1 contrast, 2 saturation, anything else none); coef (N, 9) float32: rho and sigma of
  the three operations and the three lighting shifts (dataloader.gpu_ingest.ColourParams builds both).  dst (N,) or (N, 2) int32: image n goes to
  out[dst[n]] (to both slots of its row; a slot outside `out`, e.g. -1, is skipped) of `out` (slots, 3, H, W), which must be given with
  it; slots that no image names keep their content.  With return_means
  also the (N,) contrast means the kernel used."""
  who = 'images_u8_augment'
  if not torch.is_tensor(images_u8) or images_u8.dtype != torch.uint8:
    raise TypeError('%s: images must be a uint8 tensor (got %s)' % (who, getattr(images_u8, 'dtype', type(images_u8))))
  require_gpu(images_u8, ops, coef, dst, out)
  if images_u8.dim() != 4 or images_u8.shape[3] != 3:
    raise ValueError('%s: images must be (N, H, W, 3), got %s' % (who, tuple(images_u8.shape)))
  N, H, W, _ = images_u8.shape
  if (H * W) % 4 or H * W == 0:
    raise ValueError('%s: H W = %d x %d must be a positive multiple of 4' % (who, H, W))
  for t, dt, shape, name in ((ops, torch.int32, (N, 3), 'ops'), (coef, torch.float32, (N, 9), 'coef'), (dst, torch.int32, (N,), 'dst')):
    if name == 'dst' and torch.is_tensor(t) and t.dim() == 2:
      shape = (N, 2)
    if (t is not None or name != 'dst') and (not torch.is_tensor(t) or t.dtype != dt or tuple(t.shape) != shape):
      raise ValueError('%s: %s must be %s %s, got %s %s' % (who, name, str(dt).replace('torch.', ''), shape, getattr(t, 'dtype', type(t)),
                                                            tuple(getattr(t, 'shape', ()))))
  dev = images_u8.device
  if (dst is None) != (out is None):
    raise ValueError('%s: dst and out are given together' % who)
  if out is None:
    out = torch.empty((N, 3, H, W), dtype=torch.float32, device=dev)
  else:
    require_f32c(out)
    if out.dim() != 4 or tuple(out.shape[1:]) != (3, H, W):
      raise ValueError('%s: out must be (slots, 3, %d, %d), got %s' % (who, H, W, tuple(out.shape)))
  for t, name in ((images_u8, 'images'), (ops, 'ops'), (coef, 'coef'), (dst, 'dst'), (out, 'out')):
    if t is not None and (not t.is_contiguous() or t.device != dev):
      raise TypeError('%s: %s must be contiguous and on %s' % (who, name, dev))
  means = torch.empty((N,), dtype=torch.float32, device=dev) if return_means else None
  nws = lib().mode_images_u8_augment_workspace_bytes(N, H, W)
  ws = torch.empty(max(nws // 8, 1), dtype=torch.float64, device=dev)
  with torch.cuda.device_of(images_u8), profiling.region('images_u8_augment', images_u8.numel() * 2 + 12 * N * H * W, 0, dev):
    _call('mode_images_u8_augment', ptr(images_u8), ptr(ops), ptr(coef), _optr(dst), 2 if dst is not None and dst.dim() == 2 else 1, N, H, W,
          out.shape[0], ptr(out), _optr(means), ptr(ws), nws, stream_of(images_u8))
  return (out, means) if return_means else out


def rgb_half_pil(frames_u8, tab_w, tab_h, lut, return_u8=False):
  """Panoramas 0, 1, 10, 11 of (F, 12, H, W, 3) uint8 frames halved as PIL.Image.resize((W / 2, H / 2)) halves them and normalised ->
  (F, 12, H/2, W/2) float32 (with return_u8: and the 8-bit result (F, 4, H/2, W/2, 3)) on mode_rgb_half_pil.  tab_w (W/2, 10), tab_h
  (H/2, 10): int32 device tables of dataloader.gpu_ingest.half_table_rows."""
  require_u8_frames(frames_u8, 'rgb_half_pil')
  require_gpu(tab_w, tab_h, lut)
  require_f32c(lut)
  F, _, H, W, _ = frames_u8.shape
  if H % 2 or W % 2 or H * W == 0:
    raise ValueError('rgb_half_pil: %d x %d is not even' % (H, W))
  for t, n in ((tab_w, W // 2), (tab_h, H // 2)):
    if t.dtype != torch.int32 or not t.is_contiguous() or tuple(t.shape) != (n, 10):
      raise ValueError('rgb_half_pil: a table must be contiguous int32 (%d, 10), got %s %s' % (n, t.dtype, tuple(t.shape)))
  if tuple(lut.shape) != (256, 3):
    raise ValueError('rgb_half_pil: lut %s must be (256, 3)' % (tuple(lut.shape),))
  dev = frames_u8.device
  out = torch.empty((F, 12, H // 2, W // 2), dtype=torch.float32, device=dev)
  u8 = torch.empty((F, 4, H // 2, W // 2, 3), dtype=torch.uint8, device=dev) if return_u8 else None
  with torch.cuda.device_of(frames_u8), profiling.region('rgb_half_pil', F * 4 * H * W * 3 + 4 * out.numel(), 0, dev):
    _call('mode_rgb_half_pil', ptr(frames_u8), ptr(tab_w), ptr(tab_h), ptr(lut), F, H, W, ptr(out), _optr(u8), stream_of(frames_u8))
  return (out, u8) if return_u8 else out


RESIZE_MAX_SCALE = CONSTANTS['MODE_RESIZE_MAX_SCALE']
RESIZE_MAX_TAPS = 17


def _require_windows(windows, rows, crop, shape, dev, who):
  """-> (h_win, w_win) for a window table (rows, 2) int32 on `dev` (or None: the whole image, or the crop at the top left corner)."""
  H, W = shape
  h_win, w_win = (H, W) if crop is None else (int(crop[0]), int(crop[1]))
  if not (0 < h_win <= H and 0 < w_win <= W):
    raise ValueError('%s: a window of %d x %d does not lie inside the %d x %d image' % (who, h_win, w_win, H, W))
  if windows is not None:
    if (not torch.is_tensor(windows) or windows.dtype != torch.int32 or tuple(windows.shape) != (rows, 2) or not windows.is_contiguous() or
        windows.device != dev):
      raise ValueError('%s: windows must be a contiguous int32 (%d, 2) tensor of (top, left) on %s, got %s %s' %
                       (who, rows, dev, getattr(windows, 'dtype', type(windows)), tuple(getattr(windows, 'shape', ()))))
  return h_win, w_win


def images_u8_resize_pil(images_u8, shape, tab_w, tab_h, lut=None, windows=None, per_window=1, crop=None, split=False, want_u8=True,
                         want_f32=False, out_u8=None):
  """(N, Hs, Ws, 3) uint8 images resized to shape = (H, W) as PIL.Image.resize((W, H)) resizes them, on mode_images_u8_resize_pil
  (the contract is in include/mode_hip.h) -> (u8 (N, h, w, 3) or None, f32 (N, 3, h, w) or None): the bytes and / or their lookup in
  lut, the (256, 3) normalisation table.  tab_w (W, 2 + ksize), tab_h (H, 2 + ksize): int32 device tables of
  dataloader.gpu_ingest.resize_table_rows (None for an axis whose size does not change).  windows (ceil(N / per_window), 2) int32
  device (top, left) with crop = (h, w): only that window of every resized image is computed and returned; crop alone: the window at
  (0, 0).  split: the images of a group of per_window go to slots member * (N / per_window) + group (left images first, then right ones)."""
  who = 'images_u8_resize_pil'
  if not torch.is_tensor(images_u8) or images_u8.dtype != torch.uint8:
    raise TypeError('%s: images must be a uint8 tensor (got %s)' % (who, getattr(images_u8, 'dtype', type(images_u8))))
  require_gpu(images_u8, tab_w, tab_h, lut, windows, out_u8)
  if images_u8.dim() != 4 or images_u8.shape[3] != 3 or not images_u8.is_contiguous():
    raise ValueError('%s: images must be contiguous (N, H, W, 3), got %s' % (who, tuple(images_u8.shape)))
  N, Hs, Ws, _ = images_u8.shape
  H, W = int(shape[0]), int(shape[1])
  if min(Hs, Ws, H, W) <= 0:
    raise ValueError('%s: %d x %d -> %d x %d' % (who, Hs, Ws, H, W))
  dev = images_u8.device
  per_window = int(per_window)
  if per_window < 1 or (split and N % per_window):
    raise ValueError('%s: %d images in groups of %d' % (who, N, per_window))
  h_win, w_win = _require_windows(windows, -(-N // per_window), crop, (H, W), dev, who)
  ksize = []
  for t, n, out, name in ((tab_w, Ws, W, 'tab_w'), (tab_h, Hs, H, 'tab_h')):
    if n == out:
      ksize.append(0)
      continue
    if (not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != 2 or t.shape[0] != out or not 3 <= t.shape[1] <= 2 + RESIZE_MAX_TAPS or
        not t.is_contiguous() or t.device != dev):
      raise ValueError('%s: %s must be a contiguous int32 (%d, 2 + ksize) tensor on %s, got %s %s' %
                       (who, name, out, dev, getattr(t, 'dtype', type(t)), tuple(getattr(t, 'shape', ()))))
    ksize.append(t.shape[1] - 2)
  if not (want_u8 or want_f32 or out_u8 is not None):
    raise ValueError('%s: no output asked for' % who)
  if want_f32:
    if lut is None:
      raise ValueError('%s: the float output needs lut' % who)
    require_f32c(lut)
    if tuple(lut.shape) != (256, 3) or lut.device != dev:
      raise ValueError('%s: lut %s must be (256, 3) on %s' % (who, tuple(lut.shape), dev))
  if out_u8 is not None:
    if out_u8.dtype != torch.uint8 or tuple(out_u8.shape) != (N, h_win, w_win, 3) or not out_u8.is_contiguous() or out_u8.device != dev:
      raise ValueError('%s: out_u8 must be a contiguous uint8 %s tensor on %s' % (who, (N, h_win, w_win, 3), dev))
    u8 = out_u8
  else:
    u8 = torch.empty((N, h_win, w_win, 3), dtype=torch.uint8, device=dev) if want_u8 else None
  f32 = torch.empty((N, 3, h_win, w_win), dtype=torch.float32, device=dev) if want_f32 else None
  nws = lib().mode_images_u8_resize_pil_workspace_bytes(N, Hs, Ws, H, W, h_win, w_win)
  ws = torch.empty(nws, dtype=torch.uint8, device=dev) if nws else None
  nbytes = images_u8.numel() + 2 * nws + N * h_win * w_win * ((3 if u8 is not None else 0) + (12 if f32 is not None else 0))
  with torch.cuda.device_of(images_u8), profiling.region('images_u8_resize_pil', nbytes, 0, dev):
    _call('mode_images_u8_resize_pil', ptr(images_u8), _optr(tab_w) if ksize[0] else None, ksize[0], _optr(tab_h) if ksize[1] else None, ksize[1],
          _optr(lut) if want_f32 else None, _optr(windows), per_window, 1 if split else 0, N, Hs, Ws, H, W, h_win, w_win, _optr(u8), _optr(f32), _optr(ws), nws,
          stream_of(images_u8))
  return u8, f32


def disp_resize_nearest(disp, shape, rows, cols, ratio, windows=None, crop=None):
  """(N, Hs, Ws) float32 maps -> (N, h, w): disp[n, rows[top + y], cols[left + x]] * float32(ratio) on mode_disp_resize_nearest --
  cv2.resize(..., (W, H), INTER_NEAREST) * ratio for shape = (H, W) and, with windows (N, 2) int32 (top, left) and crop = (h, w), that
  window of it.  rows (H,), cols (W,): int32 device tables of dataloader.preprocess.nearest_index_table."""
  who = 'disp_resize_nearest'
  require_gpu(disp, rows, cols, windows)
  require_f32c(disp)
  if disp.dim() != 3 or 0 in disp.shape[1:]:
    raise ValueError('%s: maps must be (N, H, W), got %s' % (who, tuple(disp.shape)))
  N, Hs, Ws = disp.shape
  H, W = int(shape[0]), int(shape[1])
  dev = disp.device
  for t, n, name in ((rows, H, 'rows'), (cols, W, 'cols')):
    if not torch.is_tensor(t) or t.dtype != torch.int32 or tuple(t.shape) != (n,) or not t.is_contiguous() or t.device != dev:
      raise ValueError('%s: %s must be a contiguous int32 (%d,) tensor on %s' % (who, name, n, dev))
  h_win, w_win = _require_windows(windows, N, crop, (H, W), dev, who)
  out = torch.empty((N, h_win, w_win), dtype=torch.float32, device=dev)
  with torch.cuda.device_of(disp), profiling.region('disp_resize_nearest', 8 * out.numel(), out.numel(), dev):
    _call('mode_disp_resize_nearest', ptr(disp), ptr(rows), ptr(cols), _optr(windows), N, Hs, Ws, H, W, h_win, w_win,
          float(ratio), ptr(out), stream_of(disp))
  return out


def _decimate2_fwd(x):
  H, W = x.shape[-2:]
  y = torch.empty(tuple(x.shape[:-2]) + ((H + 1) // 2, (W + 1) // 2), dtype=x.dtype, device=x.device)
  with torch.cuda.device_of(x), profiling.region('decimate2', 4 * (x.numel() // 2 + y.numel()), 0, x.device):
    _call('mode_decimate2', ptr(x), ptr(y), x.numel() // (H * W), H, W, stream_of(x))
  return y


def decimate2_bwd(gy, shape):
  """The adjoint of decimate2 for an input of `shape` (..., H, W): gy in the even rows and columns, +0.0 elsewhere (mode_decimate2_bwd)."""
  require_gpu(gy)
  gy = gy.contiguous()
  require_f32c(gy)
  H, W = shape[-2:]
  if tuple(gy.shape) != tuple(shape[:-2]) + ((H + 1) // 2, (W + 1) // 2):
    raise ValueError('decimate2_bwd: gradient %s does not belong to an input of shape %s' % (tuple(gy.shape), tuple(shape)))
  gx = torch.empty(tuple(shape), dtype=gy.dtype, device=gy.device)
  with torch.cuda.device_of(gy), profiling.region('decimate2_bwd', 4 * (gy.numel() + gx.numel()), 0, gy.device):
    _call('mode_decimate2_bwd', ptr(gy), ptr(gx), gx.numel() // (H * W), H, W, stream_of(gy))
  return gx


class Decimate2Function(torch.autograd.Function):

  @staticmethod
  def forward(ctx, x):
    ctx.shape = tuple(x.shape)
    return _decimate2_fwd(x)

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, gy):
    return decimate2_bwd(gy, ctx.shape)


def decimate2(x):
  """x[..., ::2, ::2] of a contiguous float32 (..., H, W) tensor, contiguous, on mode_decimate2 (the reference loader's --resize
  subsampling of the depth and confidence maps, dataloader/deep360_loader.py:147-150).  Differentiable where x requires a gradient
  (mode_decimate2_bwd); the values are the same either way."""
  require_gpu(x)
  require_f32c(x)
  if x.dim() < 2 or 0 in x.shape[-2:]:
    raise ValueError('decimate2: expected a (..., H, W) tensor with H, W > 0, got %s' % (tuple(x.shape),))
  if torch.is_grad_enabled() and x.requires_grad:
    return Decimate2Function.apply(x)
  return _decimate2_fwd(x)


# ------------------------------------------------------------------------------------ 3D60 ingest: ERP -> rectified Cassini
def _require_erp_grid(grid, N, who):
  require_gpu(grid)
  require_f32c(grid)
  if grid.dim() != 4 or grid.shape[3] != 2 or grid.shape[0] not in (1, N) or grid.shape[2] % 4 or 0 in grid.shape:
    raise ValueError('%s: grid must be (1 or %d, H, W, 2) with W a positive multiple of 4, got %s' % (who, N, tuple(grid.shape)))


def erp_pairs_u8_cassini(pairs_u8, grid, lut, flip=True, return_u8=False):
  """(N, 2, He, We, 3) uint8 ERP pairs -> the rectified Cassini pairs of the reference's 3D60 loader on mode_erp_pairs_u8_cassini
  (dataloader/dataset3D60Loader.py:177-180, 192-193, 202-205, 232-236): erp2rect_cassini(...).astype(np.uint8) of both panoramas through
  `grid` ((1 or N, H, W, 2) float32, utils.geometry.erp2rect_grid), then the stage-1 transform as a lookup in `lut` ((256, 3), the table
  of frames_u8_ingest).  -> (left, right, left_flip, right_flip, cassini_u8): (N, 3, H, W) float32 each, the flip twins None without
  `flip`, the 8-bit images (N, 2, H, W, 3) None without `return_u8`."""
  who = 'erp_pairs_u8_cassini'
  if not torch.is_tensor(pairs_u8) or pairs_u8.dtype != torch.uint8:
    raise TypeError('%s: pairs must be a uint8 tensor (got %s)' % (who, getattr(pairs_u8, 'dtype', type(pairs_u8))))
  require_gpu(pairs_u8, lut)
  if not pairs_u8.is_contiguous():
    raise TypeError('%s: pairs must be contiguous' % who)
  if pairs_u8.dim() != 5 or pairs_u8.shape[1] != 2 or pairs_u8.shape[4] != 3 or pairs_u8.shape[2] < 2 or pairs_u8.shape[3] < 2:
    raise ValueError('%s: pairs must be (N, 2, He, We, 3) with He, We >= 2, got %s' % (who, tuple(pairs_u8.shape)))
  N, _, He, We, _ = pairs_u8.shape
  _require_erp_grid(grid, N, who)
  require_f32c(lut)
  if tuple(lut.shape) != (256, 3):
    raise ValueError('%s: lut %s must be (256, 3)' % (who, tuple(lut.shape)))
  G, H, W, _ = grid.shape
  dev = pairs_u8.device
  outs = [torch.empty((N, 3, H, W), dtype=torch.float32, device=dev) for _ in range(4 if flip else 2)] + [None] * (0 if flip else 2)
  u8 = torch.empty((N, 2, H, W, 3), dtype=torch.uint8, device=dev) if return_u8 else None
  nbytes = pairs_u8.numel() + 4 * grid.numel() + sum(4 * o.numel() for o in outs if o is not None) + (0 if u8 is None else u8.numel())
  with torch.cuda.device_of(pairs_u8), profiling.region('erp_pairs_u8_cassini', nbytes, 0, dev):
    _call('mode_erp_pairs_u8_cassini', ptr(pairs_u8), ptr(grid), ptr(lut), N, He, We, H, W, G, ptr(outs[0]), ptr(outs[1]),
          _optr(outs[2]), _optr(outs[3]), _optr(u8), stream_of(pairs_u8))
  return outs[0], outs[1], outs[2], outs[3], u8


def erp_depth_disp(depth_erp, grid, cols, baseline, maxdepth, mirror=False, return_depth=False):
  """(N, He, We) float32 ERP depth -> the disparity ground truth (N, 1, H, W) of the reference's 3D60 loader on mode_erp_depth_disp
  (dataloader/dataset3D60Loader.py:182-185, 192-196, 209-210 and __depth2disp, :258-270): erp2rect_cassini through `grid`, depth above
  `maxdepth` zeroed, the sine rule on `cols` ((3, W): phi, sin(phi), cos(phi + pi / 2)), NaN where the depth is invalid.  `mirror`
  flips the re-projected depth left to right before the sine rule (the flip twin).  With return_depth also the thresholded Cassini
  depth (N, H, W)."""
  who = 'erp_depth_disp'
  require_gpu(depth_erp, cols)
  require_f32c(depth_erp, cols)
  if depth_erp.dim() != 3 or depth_erp.shape[1] < 2 or depth_erp.shape[2] < 2:
    raise ValueError('%s: depth must be (N, He, We) with He, We >= 2, got %s' % (who, tuple(depth_erp.shape)))
  N, He, We = depth_erp.shape
  _require_erp_grid(grid, N, who)
  G, H, W, _ = grid.shape
  if tuple(cols.shape) != (3, W):
    raise ValueError('%s: cols %s must be (3, %d)' % (who, tuple(cols.shape), W))
  dev = depth_erp.device
  disp = torch.empty((N, 1, H, W), dtype=torch.float32, device=dev)
  dc = torch.empty((N, H, W), dtype=torch.float32, device=dev) if return_depth else None
  nbytes = 4 * (depth_erp.numel() + grid.numel() + disp.numel() + (0 if dc is None else dc.numel()))
  with torch.cuda.device_of(depth_erp), profiling.region('erp_depth_disp', nbytes, 0, dev):
    _call('mode_erp_depth_disp', ptr(depth_erp), ptr(grid), ptr(cols), N, He, We, H, W, G, float(baseline), float(maxdepth), 1 if mirror else 0,
          ptr(disp), _optr(dc), stream_of(depth_erp))
  return (disp, dc) if return_depth else disp


# ------------------------------------------------------------------------------------ BatchNorm (+ add) (+ ReLU)
def _tag_bn(name, y):
  """Profiling label with the tensor shape (like the convolution labels), e.g. bn_train_fwd[2x32 48x256x128]."""
  return '%s[%dx%d %s]' % (name, y.shape[0], y.shape[1], 'x'.join(str(int(v)) for v in y.shape[2:])) if profiling.ENABLED else name


def _bn_ws(C, device):
  return torch.empty(lib().mode_bn_workspace_bytes(C) // 4, dtype=torch.float32, device=device)


def _written_by_kernel(*tensors):
  """The training BatchNorm kernels update running_mean / running_var / num_batches_tracked through raw pointers; torch must see those
  writes like any in-place op: the version counters move (host-side only, no launch), so that everything keyed on them -- autograd's
  saved-tensor checks, the packed-weight cache of the eval forward (_eval_wpack) -- notices."""
  live = [t for t in tensors if t is not None]
  if live:
    torch.autograd.graph.increment_version(live)
    log = getattr(_bn_tls, 'written_log', None)
    if log is not None:  # a capture is recording: the REPLAYS write these tensors too, through the same raw pointers (GraphedStep.replay)
      log.extend(live)


def written_log_begin():
  """Start recording (on this thread) the tensors the library's kernels write through raw pointers -- BatchNorm running statistics and
  batch counters; graph_step.GraphedStep calls this around a capture: every replay of the graph writes them again, with no Python in
  between to move their version counters, so replay() moves them (the packed-weight cache of the eval forward and
  GraphedStep.stale() of a captured inference otherwise miss a BatchNorm recalibration run as replayed training steps)."""
  _bn_tls.written_log = []


def written_log_end():
  log, _bn_tls.written_log = getattr(_bn_tls, 'written_log', None) or [], None
  seen, out = set(), []
  for t in log:
    if id(t) not in seen:
      seen.add(id(t))
      out.append(t)
  return out


def _bcs(t):
  B, C = t.shape[:2]
  S = t.numel() // max(B * C, 1)
  return B, C, S


def _bn_rows(t):
  """t contiguous, at an address the BatchNorm kernels take: they read rows that are multiples of 16 bytes in 16-byte pieces, so such a
  tensor starts at a multiple of 16 bytes.  A contiguous view into the middle of a buffer need not; it is copied (allocations are
  aligned), which costs a pass -- no tensor of the networks here is one."""
  if t is None:
    return None
  t = t.contiguous()
  return t.clone() if t.data_ptr() % (4 if _bcs(t)[2] % 4 else 16) else t


def bn_supported(y):
  B, C, S = _bcs(y)
  return y.is_cuda and y.dtype == torch.float32 and B * C < 65536 and B > 0  # (any S: rows that are not multiples of 16 bytes take the kernels' scalar path)


_bn_tls = threading.local()  # out_amax: the device scalar the last BnActFunction.forward of this thread asked its kernel to fill


def known_abs_max(t):
  """The largest-magnitude scalar the producer of t left next to it (BatchNorm's apply pass, bn_act), if t has not been written since."""
  tag = getattr(t, '_mode_amax', None)
  return tag[0] if tag is not None and tag[1] == t._version and tag[2] == t.data_ptr() else None


def _tag_amax(t, am):
  """Leave the maximum buffer am (or nothing, when None) next to t for known_abs_max: valid until t is written or moves."""
  if am is not None:
    t._mode_amax = (am, t._version, t.data_ptr())


def _amax_for_consumer(t, training, gradient=False):
  """The producer's side of the fp16 arithmetic: a buffer for the kernel that writes t to leave t's maximum in, when the layer that
  reads t next will want it -- else None (the plain call).  A producer knows the tensor, not the consumer's channel counts, so it asks
  by rank: a 5-D tensor feeds the 3-D stack's stride-1 layers (the `f16` argument of _conv3d_route: CONV3D_S1_F16 in a training step,
  CONV3D_EVAL_F16 in inference), a 4-D one the extractor's spherical layers (_sphere_f16_maxima's rule: 16 channels per MFMA;
  SPHERE_FWD_F16 for an activation, SPHERE_BWD_F16 for a gradient; training only).
  Kept as it was: the 3 x 3 layers' CONV2D_F16 is NOT asked here, though weight_maxima asks it -- with SPHERE_*_F16 off their operands'
  maxima come from a pass (_tagged_abs_max)."""
  if CONV_ARITH != 'bf16x6':
    return None
  if t.dim() == 5:
    want = CONV3D_S1_F16 if training else CONV3D_EVAL_F16
  else:
    want = training and (SPHERE_BWD_F16 if gradient else SPHERE_FWD_F16) and t.dim() == 4 and t.shape[1] % 16 == 0
  return torch.empty(BN_ABSMAX_FLOATS, dtype=torch.float32, device=t.device) if want else None


class BnActFunction(torch.autograd.Function):
  """out = relu?(batch_norm_train(y) [+ add]); running statistics updated in place (torch semantics)."""

  @staticmethod
  def forward(ctx, y, add, gamma, beta, running_mean, running_var, momentum, eps, relu, num_batches_tracked=None, groups=1, prestats_ws=None,
              add_carrier=None):
    ctx.add_carrier = add_carrier  # GradCarrier of `add` (the skip tensor has one other consumer), or None
    require_gpu(y, add, gamma, beta)
    y, add = _bn_rows(y), _bn_rows(add)
    require_f32c(y, gamma, beta)
    B, C, S = _bcs(y)
    out = torch.empty_like(y)
    if B % groups:
      raise RuntimeError('BatchNorm statistics groups: batch %d is not divisible by %d' % (B, groups))
    mean = torch.empty(groups * C, dtype=torch.float32, device=y.device)
    invstd = torch.empty_like(mean)
    # ReLU without a residual: the backward rebuilds the mask from y and these coefficients instead of reading `out`
    from_y = bool(relu) and add is None
    coef = torch.empty((2, groups * C), dtype=torch.float32, device=y.device) if from_y else None
    nbytes = 4 * y.numel() * (3 + (1 if add is not None else 0))
    with torch.cuda.device_of(y), profiling.region(_tag_bn('bn_train_fwd', y), nbytes, 0, y.device):
      common = (ptr(y), _optr(add), ptr(gamma), ptr(beta), _optr(running_mean), _optr(running_var), _optr(num_batches_tracked), float(momentum),
                float(eps), int(relu), ptr(out), ptr(mean), ptr(invstd), ptr(coef[0]) if from_y else None, ptr(coef[1]) if from_y else None)
      # the 3-D stack's activations feed stride-1 convolutions on the fp16 arithmetic, the extractor's the spherical layers: their
      # maximum comes out of this pass (the `_amax` entries; bn_act tags `out` with the buffer)
      _bn_tls.out_amax = out_amax = _amax_for_consumer(y, True)
      if prestats_ws is not None:  # the producing convolution left the statistics in the workspace (conv3d_bn_train): no statistics pass
        if groups != 1:
          raise RuntimeError('BatchNorm with precomputed statistics takes one statistics group')
        _call('mode_bn_train_fwd_prestats_amax', *common, ptr(prestats_ws), lib().mode_conv3d_fwd_split_stats_partials(), B, C, S,
              _optr(out_amax), stream_of(y))
      else:
        ws = _bn_ws(C * groups, y.device)
        _call('mode_bn_train_fwd_amax', *common, ptr(ws), B, C, S, groups, _optr(out_amax), stream_of(y))
    _written_by_kernel(running_mean, running_var, num_batches_tracked)
    ctx.save_for_backward(y, out if (relu and not from_y) else None, gamma, beta, mean, invstd, coef)
    ctx.relu, ctx.has_add, ctx.groups = bool(relu), add is not None, groups
    return out

  @staticmethod
  def backward(ctx, gout):
    y, out, gamma, beta, mean, invstd, coef = ctx.saved_tensors
    gout = _bn_rows(gout)
    B, C, S = _bcs(y)
    gy = torch.empty_like(y)
    need_gadd = ctx.has_add and ctx.relu and ctx.needs_input_grad[1]
    gadd = torch.empty_like(y) if need_gadd else None
    sink_g, sink_b = grad_sink(gamma), grad_sink(beta)
    fused = sink_g is not None and sink_b is not None and ctx.needs_input_grad[2] and ctx.needs_input_grad[3]
    ggamma = sink_g if fused else torch.empty_like(gamma)
    gbeta = sink_b if fused else torch.empty_like(gamma)
    # tensor passes of the two kernels: the statistics pass reads gout, y (, out); the apply pass reads them again and writes gy -- or,
    # with a skip gradient behind a ReLU, the statistics pass also writes gadd and the apply pass reads only gadd and y (3 + 1 + 2 + 1)
    if need_gadd and out is not None:
      nbytes = 4 * y.numel() * 7
    else:
      nbytes = 4 * y.numel() * (2 * (2 + (1 if out is not None else 0)) + 1 + (1 if need_gadd else 0))
    gy_amax = _amax_for_consumer(y, True, gradient=True)  # the convolution in front reads gy in both of its gradients
    with torch.cuda.device_of(y), profiling.region(_tag_bn('bn_train_bwd', y), nbytes, 0, y.device):
      ws = _bn_ws(C * ctx.groups, y.device)
      _call('mode_bn_train_bwd_amax', ptr(gout), ptr(y), _optr(out), ptr(gamma), ptr(mean), ptr(invstd), ptr(coef[0]) if coef is not None else None,
            ptr(coef[1]) if coef is not None else None, int(ctx.relu), ptr(gy), _optr(gadd), ptr(ggamma), ptr(gbeta), int(fused), ptr(ws), B, C, S,
            ctx.groups, _optr(gy_amax), stream_of(y))
    _tag_amax(gy, gy_amax)  # (survives the engine's hand-over when the tensor's Python object does; Conv3dFunction.backward computes the
    if fused:               #  maximum itself otherwise)
      ggamma = gbeta = None
    if ctx.has_add and not ctx.relu:
      gadd = gout  # the add passes the gradient through unchanged
    if gadd is not None and ctx.add_carrier is not None:
      prev = ctx.add_carrier.take(ctx)
      if prev is not None:
        gadd = gadd + prev  # (the other consumer came first: this backward cannot add inside its kernel)
      elif ctx.add_carrier.leave(gadd, ctx):
        gadd = None  # the skip's other consumer adds it inside its input-gradient kernel
    return gy, gadd, ggamma, gbeta, None, None, None, None, None, None, None, None, None


def bn_eval(y, add, gamma, beta, running_mean, running_var, eps, relu):
  require_gpu(y, add, gamma, beta, running_mean, running_var)
  y, add = _bn_rows(y), _bn_rows(add)
  require_f32c(y, gamma, beta, running_mean, running_var)
  B, C, S = _bcs(y)
  out = torch.empty_like(y)
  nbytes = 4 * y.numel() * (2 + (1 if add is not None else 0))
  with torch.cuda.device_of(y), profiling.region('bn_eval_fwd', nbytes, 0, y.device):
    _call('mode_bn_eval_fwd', ptr(y), _optr(add), ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var), float(eps),
          int(relu), ptr(out), B, C, S, stream_of(y))
  return out


def bn_act(bn, y, add=None, relu=False, groups=1, add_carrier=None):
  """groups > 1: batch statistics per group of B / groups consecutive samples, as `groups` consecutive calls would take them.
  nn.BatchNorm2d/3d `bn` applied to y, then the optional residual add and ReLU, in one fused pass (two in training).
  Same state handling as nn.BatchNorm: train mode uses batch statistics and updates running_mean / running_var /
  num_batches_tracked; eval mode uses the running statistics."""
  use_batch_stats = bn.training or bn.running_mean is None
  if use_batch_stats:
    momentum = bn.momentum
    update = bn.training and bn.track_running_stats
    nbt = bn.num_batches_tracked if update else None
    if groups > 1 and momentum is None:
      raise NotImplementedError('grouped BatchNorm statistics need a fixed momentum')
    if nbt is not None and (momentum is None or not (nbt.is_cuda and nbt.dtype == torch.int64)):
      nbt.add_(groups)  # cumulative moving average needs the count on the host; otherwise the kernel counts the batches
      if momentum is None:
        momentum = 1.0 / float(nbt)
      nbt = None
    if add_carrier is not None:
      add_carrier.arm(add is not None and add.requires_grad and torch.is_grad_enabled())
    out = BnActFunction.apply(y, add, bn.weight, bn.bias, bn.running_mean if update else None, bn.running_var if update else None,
                              momentum if momentum is not None else 0.0, bn.eps, relu, nbt, groups, None, add_carrier)
    am = getattr(_bn_tls, 'out_amax', None)
    if am is not None:
      _bn_tls.out_amax = None
      _tag_amax(out, am)  # (a later in-place write to `out` invalidates it: known_abs_max checks)
    return out
  if torch.is_grad_enabled() and (y.requires_grad or bn.weight.requires_grad):
    # eval-mode BN inside a graph that needs gradients: rare (the reference never does it); vendor ops keep autograd correct
    out = torch.nn.functional.batch_norm(y, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
    out = out + add if add is not None else out
    return torch.relu(out) if relu else out
  return bn_eval(y, add, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, relu)


# ------------------------------------------------------------------------------------ classifier head in training, fused
# classifN = Sequential(convbn_3d(32, 32), ReLU, Conv3d(32, 1)) (mode_disparity.py:76-80): from the first convolution's output on --
# BatchNorm (batch statistics) + ReLU + the 32 -> 1 convolution + the residual add of mode_disparity.py:128-129 -- as ONE operator whose
# activated intermediate never reaches HBM (csrc/classif_head.hip: 5 passes over the 403 MB tensor per head and step instead of 13).
CLASSIF_FUSED = True  # bench.py --no-fused-classif measures the composition of separate operators


def classif_fused_supported(y, bn, conv):
  """y = output of the first convolution; bn = its BatchNorm3d (training mode); conv = the single-channel Conv3d behind the ReLU."""
  return (CLASSIF_FUSED and y.is_cuda and y.dtype == torch.float32 and y.dim() == 5 and y.shape[0] > 0 and y.shape[1] <= 32 and
          bn.training and bn.momentum is not None and bn.weight is not None and bn.bias is not None and
          type(conv) is torch.nn.Conv3d and conv.out_channels == 1 and conv.in_channels == y.shape[1] and conv.bias is None and
          tuple(conv.kernel_size) == (3, 3, 3) and tuple(conv.stride) == (1, 1, 1) and tuple(conv.padding) == (1, 1, 1) and
          tuple(conv.dilation) == (1, 1, 1) and conv.groups == 1 and conv.padding_mode == 'zeros' and
          y.shape[1] * y.shape[2] * y.shape[3] * y.shape[4] < 2**30)


class ClassifHeadFunction(torch.autograd.Function):
  """cost = conv3d(relu(batch_norm_train(y)), w) [+ add]; running statistics updated in place (torch semantics)."""

  @staticmethod
  def forward(ctx, y, w, gamma, beta, add, running_mean, running_var, momentum, eps, num_batches_tracked):
    require_gpu(y, w, gamma, beta, add)
    y, w = y.contiguous(), w.contiguous()
    add = add.contiguous() if add is not None else None
    require_f32c(y, w, gamma, beta)
    B, C, D, H, W = y.shape
    cost = torch.empty((B, 1, D, H, W), dtype=y.dtype, device=y.device)
    if add is not None:
      require_f32c(add)
      if tuple(add.shape) != tuple(cost.shape):
        raise RuntimeError('classifier head: residual %s does not match the output %s' % (tuple(add.shape), tuple(cost.shape)))
    saved = torch.empty((4, C), dtype=torch.float32, device=y.device)  # mean, invstd, scale, shift
    with torch.cuda.device_of(y), profiling.region(_tag3('classif_fwd', C, 1, 1, D, H, W), 4 * (2 * y.numel() + cost.numel() * (2 if add is not None else 1)),
                                                   2 * cost.numel() * C * 27, y.device):
      ws = torch.empty(max(lib().mode_classif_workspace_bytes(B, C, D, H, W) // 4, 1), dtype=torch.float32, device=y.device)
      _call('mode_classif_train_fwd', ptr(y), ptr(gamma), ptr(beta), _optr(running_mean), _optr(running_var), _optr(num_batches_tracked),
            float(momentum), float(eps), ptr(w), _optr(add), ptr(cost), ptr(saved[0]), ptr(saved[1]), ptr(saved[2]), ptr(saved[3]), ptr(ws), B, C, D,
            H, W, stream_of(y))
    _written_by_kernel(running_mean, running_var, num_batches_tracked)
    ctx.save_for_backward(y, w, gamma, beta, saved)
    ctx.has_add = add is not None
    return cost

  @staticmethod
  def backward(ctx, gcost):
    y, w, gamma, beta, saved = ctx.saved_tensors
    gcost = gcost.contiguous()
    B, C, D, H, W = y.shape
    gy = torch.empty_like(y)
    sink_w = grad_sink(w) if ctx.needs_input_grad[1] else None
    sink_g, sink_b = grad_sink(gamma), grad_sink(beta)
    fused = sink_w is not None and sink_g is not None and sink_b is not None and ctx.needs_input_grad[2] and ctx.needs_input_grad[3]
    gw = sink_w if fused else torch.empty_like(w)
    ggamma = sink_g if fused else torch.empty_like(gamma)
    gbeta = sink_b if fused else torch.empty_like(beta)
    with torch.cuda.device_of(y), profiling.region(_tag3('classif_bwd', C, 1, 1, D, H, W), 4 * (3 * y.numel() + 4 * gcost.numel()),
                                                   2 * 3 * gcost.numel() * C * 27, y.device):
      ws = torch.empty(max(lib().mode_classif_workspace_bytes(B, C, D, H, W) // 4, 1), dtype=torch.float32, device=y.device)
      gy_amax = _amax_for_consumer(y, True, gradient=True)  # the 32 -> 32 convolution in front reads gy in both of its gradients (BnActFunction.backward)
      _call('mode_classif_train_bwd_amax', ptr(gcost), ptr(y), ptr(w), ptr(gamma), ptr(beta), ptr(saved[0]), ptr(saved[1]), ptr(saved[2]),
            ptr(saved[3]), ptr(gy), ptr(gw), ptr(ggamma), ptr(gbeta), int(fused), ptr(ws), B, C, D, H, W, _optr(gy_amax), stream_of(y))
      _tag_amax(gy, gy_amax)
    if fused:
      gw = ggamma = gbeta = None
    return gy, gw, ggamma, gbeta, (gcost if ctx.has_add else None), None, None, None, None, None


def classif_head_train(y, bn, conv, add=None):
  """relu(bn(y)) -> conv (32 -> 1) [+ add] in training mode, fused (classif_fused_supported(y, bn, conv) must hold)."""
  update = bn.training and bn.track_running_stats
  nbt = bn.num_batches_tracked if update else None
  if nbt is not None and not (nbt.is_cuda and nbt.dtype == torch.int64):
    nbt.add_(1)
    nbt = None
  return ClassifHeadFunction.apply(y, conv.weight, bn.weight, bn.bias, add, bn.running_mean if update else None,
                                   bn.running_var if update else None, bn.momentum, bn.eps, nbt)


# ------------------------------------------------------------------------------------ spatial pyramid pooling (conv='Regular' extractor)
SPP_KERNELS = (8, 16, 32, 64)  # the levels of csrc/spp.hip, in the order of its arguments (branch4, branch3, branch2, branch1 of the reference)


def _spp_plane(t, who):
  if t.dim() != 4:
    raise ValueError('%s takes (N, C, H, W) tensors (got %s)' % (who, tuple(t.shape)))


class SppPoolFunction(torch.autograd.Function):
  """The four nn.AvgPool2d((k, k), stride=(k, k)), k = 8, 16, 32, 64, of the SPP branches (submodule.py:228-246) in one pass over
  `skip` (mode_spp_pool_fwd).  Fifth output: `skip` itself, for its other consumer -- the concatenation.  That way both gradients of
  `skip` arrive HERE, and the backward writes their sum in one pass (mode_spp_pool_bwd: the slice of the concatenation's gradient,
  read where it lies, plus the four broadcast block gradients) instead of a slice copy and four adds by autograd."""

  @staticmethod
  def forward(ctx, skip):
    require_gpu(skip)
    _spp_plane(skip, 'spp_pool')
    require_f32c(skip)
    N, C, H, W = skip.shape
    ys = tuple(torch.empty((N, C, H // k, W // k), dtype=skip.dtype, device=skip.device) for k in SPP_KERNELS)
    with torch.cuda.device_of(skip), profiling.region('spp_pool_fwd[%dx%d]' % (H, W) if profiling.ENABLED else 'spp_pool_fwd',
                                                      4 * (skip.numel() + sum(y.numel() for y in ys)), 0, skip.device):
      _call('mode_spp_pool_fwd', ptr(skip), ptr(ys[0]), ptr(ys[1]), ptr(ys[2]), ptr(ys[3]), N * C, H, W, stream_of(skip))
    ctx.shape = tuple(skip.shape)
    ctx.set_materialize_grads(False)
    return ys + (skip,)

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, g8, g16, g32, g64, gslice):
    N, C, H, W = ctx.shape
    gs = [g8, g16, g32, g64]
    like = next((g for g in gs + [gslice] if g is not None), None)
    if like is None:
      return None
    for i, k in enumerate(SPP_KERNELS):
      gs[i] = torch.zeros((N, C, H // k, W // k), dtype=like.dtype, device=like.device) if gs[i] is None else gs[i].contiguous()
    Cg = C
    if gslice is not None:
      st = gslice.stride()
      if N == 1 and st[1:] == (H * W, W, 1):
        pass  # one sample: channels c of a (1, C', H, W) tensor lie where a (1, C, H, W) one has them
      elif st[1:] == (H * W, W, 1) and st[0] % (H * W) == 0 and st[0] >= C * H * W:
        Cg = st[0] // (H * W)  # C consecutive channels of a contiguous (N, Cg, H, W) tensor: read in place
      else:
        gslice = gslice.contiguous()
    require_gpu(like)
    require_f32c(*gs)
    if gslice is not None and gslice.dtype != torch.float32:
      raise TypeError('libmode_hip kernels are fp32 (got %s)' % gslice.dtype)
    gskip = torch.empty((N, C, H, W), dtype=like.dtype, device=like.device)
    nbytes = 4 * (gskip.numel() * (2 if gslice is not None else 1) + sum(g.numel() for g in gs))
    with torch.cuda.device_of(gskip), profiling.region('spp_pool_bwd[%dx%d]' % (H, W) if profiling.ENABLED else 'spp_pool_bwd', nbytes, 0,
                                                       gskip.device):
      _call('mode_spp_pool_bwd', _optr(gslice), Cg, 0, ptr(gs[0]), ptr(gs[1]), ptr(gs[2]), ptr(gs[3]), ptr(gskip), N, C, H, W, stream_of(gskip))
    return gskip


class SppPooled(tuple):
  """The four pooled tensors (k = 8, 16, 32, 64); `.skip` is the input as SppPoolFunction hands it on -- pass it to spp_concat in
  place of the original, so that the gradient of `skip` is written in one pass."""
  skip = None


def spp_pool(skip):
  """(pool8, pool16, pool32, pool64) of skip (N, C, H, W), H and W >= 64: nn.AvgPool2d((k, k), stride=(k, k)) each, floor semantics."""
  out = SppPoolFunction.apply(skip)
  pooled = SppPooled(out[:4])
  pooled.skip = out[4]
  return pooled


class SppConcatFunction(torch.autograd.Function):
  """torch.cat((raw, skip, up(b4), up(b3), up(b2), up(b1)), 1) with up = F.interpolate(size=skip's, mode='bilinear',
  align_corners=True) (submodule.py:253-266) as one launch (mode_spp_concat_fwd).  Backward (mode_spp_concat_bwd): raw's gradient as a
  contiguous copy, the branch gradients by the adjoint of the upsampling in gather form (no atomics); skip's gradient is the slice
  of the incoming gradient, returned as a VIEW -- SppPoolFunction's backward reads it in place."""

  @staticmethod
  def forward(ctx, raw, skip, b4, b3, b2, b1):
    ts = (raw, skip, b4, b3, b2, b1)
    require_gpu(*ts)
    for t in ts:
      _spp_plane(t, 'spp_concat')
    require_f32c(*ts)
    N, Cs, H, W = skip.shape
    Cr, Cb = raw.shape[1], b4.shape[1]
    if tuple(raw.shape) != (N, Cr, H, W):
      raise ValueError('spp_concat: raw %s does not match skip %s' % (tuple(raw.shape), tuple(skip.shape)))
    for b, k in zip((b4, b3, b2, b1), SPP_KERNELS):
      if tuple(b.shape) != (N, Cb, H // k, W // k):
        raise ValueError('spp_concat: the k = %d branch is %s, expected %s' % (k, tuple(b.shape), (N, Cb, H // k, W // k)))
    out = torch.empty((N, Cr + Cs + 4 * Cb, H, W), dtype=skip.dtype, device=skip.device)
    with torch.cuda.device_of(skip), profiling.region('spp_concat_fwd[%dx%d]' % (H, W) if profiling.ENABLED else 'spp_concat_fwd',
                                                      4 * (raw.numel() + skip.numel() + out.numel()), 0, skip.device):
      _call('mode_spp_concat_fwd', ptr(raw), ptr(skip), ptr(b4), ptr(b3), ptr(b2), ptr(b1), ptr(out), N, Cr, Cs, Cb, H, W, stream_of(skip))
    ctx.dims = (N, Cr, Cs, Cb, H, W)
    return out

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, gcat):
    N, Cr, Cs, Cb, H, W = ctx.dims
    require_gpu(gcat)
    gcat = gcat.contiguous()
    require_f32c(gcat)
    graw = torch.empty((N, Cr, H, W), dtype=gcat.dtype, device=gcat.device)
    gbs = [torch.empty((N, Cb, H // k, W // k), dtype=gcat.dtype, device=gcat.device) for k in SPP_KERNELS]
    nbytes = 4 * (2 * graw.numel() + 4 * N * Cb * H * W + sum(g.numel() for g in gbs))
    with torch.cuda.device_of(gcat), profiling.region('spp_concat_bwd[%dx%d]' % (H, W) if profiling.ENABLED else 'spp_concat_bwd', nbytes, 0,
                                                      gcat.device):
      _call('mode_spp_concat_bwd', ptr(gcat), ptr(graw), ptr(gbs[0]), ptr(gbs[1]), ptr(gbs[2]), ptr(gbs[3]), N, Cr, Cs, Cb, H, W, stream_of(gcat))
    return (graw, gcat[:, Cr:Cr + Cs]) + tuple(gbs)


def spp_concat(raw, skip, b4, b3, b2, b1):
  """(N, Cr + Cs + 4 Cb, H, W): raw, skip and the branch outputs b4 (k = 8), b3 (16), b2 (32), b1 (64) upsampled to (H, W), concatenated
  in the reference's order.  `skip`: SppPooled.skip when the branches come from spp_pool of the same tensor."""
  return SppConcatFunction.apply(raw, skip, b4, b3, b2, b1)


# ------------------------------------------------------------------------------------ fusion network: pooling, 2x2 transposed conv, head
class MaxPool2x2Function(torch.autograd.Function):
  """nn.MaxPool2d(2, stride=2) (mode_fusion.py:146, :161, :190) on csrc/fusion_ops.hip; the backward recomputes the picks from x."""

  @staticmethod
  def forward(ctx, x):
    require_gpu(x)
    x = x.contiguous()
    require_f32c(x)
    B, C, H, W = x.shape
    y = torch.empty((B, C, H // 2, W // 2), dtype=x.dtype, device=x.device)
    with torch.cuda.device_of(x), profiling.region('maxpool2x2_fwd', 4 * (x.numel() + y.numel()), 0, x.device):
      _call('mode_maxpool2x2_fwd', ptr(x), ptr(y), B * C, H, W, stream_of(x))
    ctx.save_for_backward(x)
    return y

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, gy):
    x, = ctx.saved_tensors
    gy = gy.contiguous()
    B, C, H, W = x.shape
    gx = torch.empty_like(x)
    with torch.cuda.device_of(x), profiling.region('maxpool2x2_bwd', 4 * (2 * x.numel() + gy.numel()), 0, x.device):
      _call('mode_maxpool2x2_bwd', ptr(x), ptr(gy), ptr(gx), B * C, H, W, stream_of(x))
    return gx


def maxpool2x2_supported(x, pool):
  ks = pool.kernel_size if isinstance(pool.kernel_size, tuple) else (pool.kernel_size,) * 2
  st = pool.stride if isinstance(pool.stride, tuple) else (pool.stride,) * 2
  pad = pool.padding if isinstance(pool.padding, tuple) else (pool.padding,) * 2
  dil = pool.dilation if isinstance(pool.dilation, tuple) else (pool.dilation,) * 2
  return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and ks == (2, 2) and st == (2, 2) and pad == (0, 0) and dil == (1, 1) and
          not pool.ceil_mode and not pool.return_indices and x.shape[2] >= 2 and x.shape[3] >= 2)


def maxpool2x2(x):
  return MaxPool2x2Function.apply(x)


def _deconv2x2_gemm(x, w):
  """y4 (B, 4 Co, H, W) = the 1x1 convolution half of ConvTranspose2d(Ci, Co, 2, 2): row 4 o + 2 i + j of the weight's own (Ci, 4 Co)
  storage -- mode_conv1x1_bwd_data reads a (rows-of-the-reduction, output) weight exactly as w lies."""
  B, Ci, H, W = x.shape
  R = w.shape[1] * 4
  y4 = torch.empty((B, R, H, W), dtype=x.dtype, device=x.device)
  with torch.cuda.device_of(x), profiling.region(_tag1('deconv2x2_gemm', Ci, R, 1, H, W), 4 * (x.numel() + y4.numel() + w.numel()),
                                                 2 * y4.numel() * Ci, x.device):
    wp = torch.empty(lib().mode_conv1x1_wpack_bytes(R, Ci) // 4, dtype=torch.float32, device=x.device)
    _call('mode_conv1x1_bwd_data', ptr(x), ptr(w), ptr(y4), ptr(wp), B, R, H, W, Ci, 1, stream_of(x))
  return y4


def _depth_to_space2(y4, scale, shift, relu):
  B, R, H, W = y4.shape
  Co = R // 4
  y = torch.empty((B, Co, 2 * H, 2 * W), dtype=y4.dtype, device=y4.device)
  with torch.cuda.device_of(y4), profiling.region('depth_to_space2', 8 * y4.numel(), 0, y4.device):
    _call('mode_depth_to_space2', ptr(y4), _optr(scale), _optr(shift), ptr(y), B, Co, H, W, int(relu), stream_of(y4))
  return y


def deconv2x2_supported(x, conv):
  """nn.ConvTranspose2d(Ci, Co, 2, 2) of the fusion decoder (mode_fusion.py:195, :212): kernel 2, stride 2, no padding; the 1x1 GEMM's
  weight gradient loads 16-byte row pieces (W % 4 == 0)."""
  return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and type(conv) is torch.nn.ConvTranspose2d and conv.kernel_size == (2, 2) and
          conv.stride == (2, 2) and conv.padding == (0, 0) and conv.output_padding == (0, 0) and conv.dilation == (1, 1) and conv.groups == 1 and
          x.shape[3] % 4 == 0 and 4 * max(conv.in_channels, conv.out_channels) * x.shape[2] * x.shape[3] < 2**31)


class Deconv2x2Function(torch.autograd.Function):
  """y = conv_transpose2d(x, w (Ci, Co, 2, 2), bias, stride 2): the 1x1 GEMM on csrc/conv1x1.hip + the rearrangement of fusion_ops.hip."""

  @staticmethod
  def forward(ctx, x, w, bias):
    require_gpu(x, w)
    x, w = x.contiguous(), w.contiguous()
    require_f32c(x, w)
    ctx.save_for_backward(x, w)
    ctx.has_bias = bias is not None
    return _depth_to_space2(_deconv2x2_gemm(x, w), None, bias.contiguous() if bias is not None else None, False)

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, gy):
    x, w = ctx.saved_tensors
    gy = gy.contiguous()
    B, Ci, H, W = x.shape
    Co = w.shape[1]
    R = 4 * Co
    g4 = torch.empty((B, R, H, W), dtype=gy.dtype, device=gy.device)
    with torch.cuda.device_of(gy), profiling.region('space_to_depth2', 8 * gy.numel(), 0, gy.device):
      _call('mode_space_to_depth2', ptr(gy), ptr(g4), B, Co, H, W, stream_of(gy))
    gx = gw = gb = None
    if ctx.needs_input_grad[0]:  # gx[b, c, q] = sum_r w[c][r] g4[b, r, q]: a 1x1 convolution R -> Ci with the weight as it lies
      gx = torch.empty_like(x)
      with torch.cuda.device_of(x), profiling.region(_tag1('deconv2x2_bwd_data', R, Ci, 1, H, W), 4 * (gx.numel() + g4.numel() + w.numel()),
                                                     2 * g4.numel() * Ci, x.device):
        wp = torch.empty(lib().mode_conv1x1_wpack_bytes(R, Ci) // 4, dtype=torch.float32, device=x.device)
        _call('mode_conv1x1_fwd', ptr(g4), ptr(w), ptr(gx), ptr(wp), B, R, H, W, Ci, 1, stream_of(x))
    if ctx.needs_input_grad[1]:  # gw[c][r] = sum x[b, c, q] g4[b, r, q]: the 1x1 weight gradient with "gy" := x, "x" := g4
      sink = grad_sink(w)
      gw = sink if sink is not None else torch.empty_like(w)
      with torch.cuda.device_of(x), profiling.region(_tag1('deconv2x2_bwd_weight', R, Ci, 1, H, W), 4 * (x.numel() + g4.numel() + w.numel()),
                                                     2 * g4.numel() * Ci, x.device):
        ws = torch.empty(max(lib().mode_conv1x1_bwd_weight_workspace_bytes(B, R, H, W, Ci, 1) // 4, 1), dtype=torch.float32, device=x.device)
        _call('mode_conv1x1_bwd_weight', ptr(x), ptr(g4), ptr(gw), ptr(ws), B, R, H, W, Ci, 1, int(sink is not None), stream_of(x))
      if sink is not None:
        gw = None
    if ctx.has_bias and ctx.needs_input_grad[2]:
      gb = gy.sum((0, 2, 3))
    return gx, gw, gb


def deconv2x2(x, conv):
  return Deconv2x2Function.apply(x, conv.weight, conv.bias)


def deconv2x2_bn_eval(x, conv, bn, relu):
  """relu?(eval-mode bn(conv_transpose2d(x))) in two launches: the 1x1 GEMM, then the rearrangement with bias and BatchNorm folded into
  its per-channel affine (C-element vectors, formed on the device)."""
  x, w = x.contiguous(), conv.weight.detach().contiguous()
  require_gpu(x, w)
  require_f32c(x, w)
  scale = bn.weight.detach() * torch.rsqrt(bn.running_var + bn.eps)
  bias = conv.bias.detach() if conv.bias is not None else torch.zeros_like(bn.running_mean)
  shift = (bias - bn.running_mean) * scale + bn.bias.detach()
  return _depth_to_space2(_deconv2x2_gemm(x, w), scale.contiguous(), shift.contiguous(), relu)


def conv1x1_sigmoid_supported(x, conv):
  """nn.Conv2d(C, 1, 1, bias=True) + nn.Sigmoid, the last two layers of the fusion network (mode_fusion.py:228-229)."""
  return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and type(conv) is torch.nn.Conv2d and conv.kernel_size == (1, 1) and
          conv.stride == (1, 1) and conv.padding == (0, 0) and conv.groups == 1 and conv.out_channels == 1 and conv.in_channels <= 64 and
          (x.shape[2] * x.shape[3]) % 4 == 0)


class Conv1x1SigmoidFunction(torch.autograd.Function):

  @staticmethod
  def forward(ctx, x, w, bias):
    require_gpu(x, w)
    x, w = x.contiguous(), w.contiguous()
    require_f32c(x, w)
    B, C, H, W = x.shape
    s = torch.empty((B, 1, H, W), dtype=x.dtype, device=x.device)
    with torch.cuda.device_of(x), profiling.region('conv1x1_sigmoid_fwd', 4 * (x.numel() + s.numel()), 2 * x.numel(), x.device):
      _call('mode_conv1x1_sigmoid_fwd', ptr(x), ptr(w), _optr(bias), ptr(s), B, C, H * W, stream_of(x))
    ctx.save_for_backward(x, w, s)
    ctx.has_bias = bias is not None
    return s

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, gs):
    x, w, s = ctx.saved_tensors
    gs = gs.contiguous()
    B, C, H, W = x.shape
    gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
    gw = torch.empty_like(w)
    gb = torch.empty(1, dtype=x.dtype, device=x.device) if ctx.has_bias else None
    with torch.cuda.device_of(x), profiling.region('conv1x1_sigmoid_bwd', 4 * (3 * x.numel() + 2 * s.numel()), 4 * x.numel(), x.device):
      ws = torch.empty(max(lib().mode_conv1x1_sigmoid_bwd_workspace_bytes(B, H * W) // 4, 1), dtype=torch.float32, device=x.device)
      _call('mode_conv1x1_sigmoid_bwd', ptr(x), ptr(w), ptr(s), ptr(gs), _optr(gx), ptr(gw), _optr(gb), 0, ptr(ws), B, C, H * W, stream_of(x))
    return gx, gw if ctx.needs_input_grad[1] else None, gb if (ctx.has_bias and ctx.needs_input_grad[2]) else None


def conv1x1_sigmoid(x, conv):
  return Conv1x1SigmoidFunction.apply(x, conv.weight, conv.bias)


# ------------------------------------------------------------------------------------ eval mode: convolution + folded BatchNorm
# In inference every convbn / convbn_3d / sphereConvbn block (models/submodule.py:15-22, 61-74) is ONE launch: the BatchNorm
# scale goes into the packed weights, shift / residual add / ReLU into the store of the convolution kernel (the *_bn entry points
# of include/mode_hip.h).  No BatchNorm launch is left in an eval forward, and the un-normalised convolution result never
# reaches HBM.
def bn_foldable(bn, y_like=None):
  """Eval-mode BatchNorm with running statistics and affine parameters, fp32 on the GPU."""
  return (not bn.training and bn.running_mean is not None and bn.weight is not None and bn.bias is not None and bn.weight.is_cuda and
          bn.weight.dtype == torch.float32 and not torch.is_grad_enabled())


# ------------------------------------------------------------------------------------ packed weights of the eval forward, kept per layer
# Every forward entry repacks its weights (with the folded BatchNorm scale) into the `wpack` workspace before it runs: 113 small
# launches, 0.65 ms of the 10.3 ms eval forward at one pair (profiles/r04_eval_b1_kernel_stats.txt).  In eval mode the weights do not
# change between calls, so the *_bn_eval operators keep the workspace ON THE BatchNorm MODULE of the layer (it dies with the model:
# no stale hit through a recycled address), keyed on the entry, the arithmetic and (data_ptr, _version) of the weight and of the four
# BatchNorm tensors -- an optimizer step, load_state_dict or running-statistics update bumps a version and the next call repacks (the
# library's own training kernels write the running statistics through raw pointers and bump the counters themselves: _written_by_kernel).
# Writes through `.data` are invisible to the counters: invalidate_eval_packs(module) after those.  On a hit the entry runs under
# mode_weight_pack_reuse(1) (include/mode_hip.h) and skips its pack kernels.  A hipGraph captured from a forward that hit the cache
# replays WITHOUT pack kernels: GraphedStep records the versions the hits relied on and refuses to replay once one has moved.
EVAL_PACK_CACHE = True


class _PackReuse(object):

  def __init__(self, on):
    self.on = on

  def __enter__(self):
    if self.on:
      lib().mode_weight_pack_reuse(1)

  def __exit__(self, *exc):
    if self.on:
      lib().mode_weight_pack_reuse(0)
    return False


_pack_tls = threading.local()


def frozen_packs_begin():
  """Start recording which (tensor, version) pairs the packed-weight cache vouches for on this thread (graph_step.GraphedStep calls this
  around a capture): a captured eval forward that HITS the cache has no pack kernels in its graph -- its replays read the workspaces as
  they were at capture time, so they are only valid while those versions stand."""
  _pack_tls.log = []


def frozen_packs_end():
  log, _pack_tls.log = getattr(_pack_tls, 'log', None) or [], None
  return log


def invalidate_eval_packs(module):
  """Drop every packed-weight workspace kept under `module`.  Needed only after writes torch cannot see -- `param.data.copy_()`,
  `.data.mul_()`, raw-pointer writes from foreign code -- which do not move a version counter; optimizer steps, load_state_dict, in-place
  torch ops and this library's own training kernels are noticed without it."""
  for m in module.modules():
    m.__dict__.pop('_mode_hip_packed', None)


def _eval_wpack(bn, tag, w, nfloats, device):
  """(workspace, context manager to run the entry under): a kept workspace + pack reuse on a hit, a fresh one otherwise."""
  capturing = torch.cuda.is_current_stream_capturing()
  # replicas of nn.DataParallel share the original module's __dict__ entries (a shallow copy) but hold freshly broadcast parameters at
  # recycled addresses with version 0: no cache for them (train_disparity.py:264-265 only ever runs replicas in training anyway)
  if not EVAL_PACK_CACHE or bn is None or getattr(bn, '_is_replica', False):
    return torch.empty(nfloats, dtype=torch.float32, device=device), _PackReuse(False)
  tens = (w, bn.weight, bn.bias, bn.running_mean, bn.running_var)
  key = (tag, CONV_ARITH, nfloats, str(device), tuple(w.shape)) + tuple((t.data_ptr(), t._version) if t is not None else None for t in tens)
  cache = bn.__dict__.setdefault('_mode_hip_packed', {})
  wp = cache.get(key)
  if wp is not None:
    if capturing:  # a live graph now reads this workspace: it stays for the lifetime of the layer
      bn.__dict__.setdefault('_mode_hip_packed_pinned', []).append(wp)
      log = getattr(_pack_tls, 'log', None)
      if log is not None:
        log.extend((t, t._version) for t in tens if t is not None)
    return wp, _PackReuse(True)
  wp = torch.empty(nfloats, dtype=torch.float32, device=device)
  if not capturing:  # (memory of a capture belongs to the graph's pool: not kept)
    if len(cache) >= 4:
      cache.clear()
    cache[key] = wp
  return wp, _PackReuse(False)


def _epilogue(bn, add, relu, out):
  """(ctypes struct, tensors to keep alive): `add` must have the layout of `out`."""
  keep = [bn.weight.detach().contiguous(), bn.bias.detach().contiguous(), bn.running_mean.contiguous(), bn.running_var.contiguous()]
  if add is not None:
    add = add.contiguous()
    require_gpu(add)
    require_f32c(add)
    if tuple(add.shape) != tuple(out.shape):
      raise RuntimeError('residual input %s does not match the output %s' % (tuple(add.shape), tuple(out.shape)))
    keep.append(add)
  e = BnEpilogue(ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), float(bn.eps), _optr(add), int(bool(relu)))
  return e, keep


def _optr(t):
  return ptr(t) if t is not None else None


def conv3d_bn_eval(x, w, bn, stride=1, add=None, relu=False):
  """relu?(bn(conv3d(x, w, stride, padding 1)) [+ add]) with bn in eval mode; Co > 1."""
  require_gpu(x, w)
  x, w = x.contiguous(), w.detach().contiguous()
  require_f32c(x, w)
  B, Ci, D, H, W = x.shape
  Co = w.shape[0]
  y = torch.empty((B, Co, _out3(D, stride), _out3(H, stride), _out3(W, stride)), dtype=x.dtype, device=x.device)
  e, keep = _epilogue(bn, add, relu, y)
  flops = 2 * y.numel() * Ci * 27
  with torch.cuda.device_of(x), profiling.region(_tag3('conv3d_bn_eval', Ci, Co, stride, D, H, W), 4 * (x.numel() + y.numel() + w.numel()),
                                                 flops, x.device):
    route = _conv3d_route(Ci, Co, stride, 0, (D, H, W), CONV3D_EVAL_F16)
    tag = {'f32': 'conv3d_fwd_bn s%d' % stride, 'split': 'conv3d_fwd_split', 'split_f16': 'conv3d_fwd_split_f16_bn', 's2_split': 'conv3d_fwd_s2_split'}
    wp, reuse = _eval_wpack(bn, tag[route], w, lib().mode_conv3d_wpack_bytes(Ci, Co) // 4, x.device)
    ax = ay = None
    if route == 'split_f16':
      # two fp16 pieces (round 6): the input's maximum is the tag the producing eval kernel left (this one: y's below), else a pass;
      # the folded weights' maximum is taken inside the call, with the pack, and lives in the kept workspace
      ax, ay = _tagged_abs_max(x), torch.empty(BN_ABSMAX_FLOATS, dtype=torch.float32, device=x.device)
    elif route == 's2_split':  # (the stride-1 layer behind it runs on the fp16 arithmetic: its operand maximum out of this epilogue)
      ay = _amax_for_consumer(y, False)
    tail = (ptr(wp), B, Ci, D, H, W, Co)
    with reuse:
      if route == 'split_f16':
        _call('mode_conv3d_fwd_split_f16_bn', ptr(x), ptr(w), ptr(ax), ctypes.byref(e), ptr(y), ptr(ay), *tail, stream_of(x))
      elif route == 'split':
        _call('mode_conv3d_fwd_split', ptr(x), ptr(w), ctypes.byref(e), ptr(y), *tail, stream_of(x))
      elif route == 's2_split':
        _call('mode_conv3d_fwd_s2_split_amax', ptr(x), ptr(w), ctypes.byref(e), ptr(y), _optr(ay), *tail, stream_of(x))
      else:
        _call('mode_conv3d_fwd_bn', ptr(x), ptr(w), ctypes.byref(e), ptr(y), *tail, stride, stream_of(x))
    _tag_amax(y, ay)
  return y


def deconv3d_bn_eval(x, w, bn, add=None, relu=False):
  require_gpu(x, w)
  x, w = x.contiguous(), w.detach().contiguous()
  require_f32c(x, w)
  B, Cin, D, H, W = x.shape
  Cout = w.shape[1]
  y = torch.empty((B, Cout, 2 * D, 2 * H, 2 * W), dtype=x.dtype, device=x.device)
  e, keep = _epilogue(bn, add, relu, y)
  flops = 2 * x.numel() * Cout * 27
  with torch.cuda.device_of(x), profiling.region('deconv3d_bn_eval', 4 * (x.numel() + y.numel() + w.numel()), flops, x.device):
    # (round 5: the split kernel with its own epilogue instantiation -- residual values of four channels requested ahead of their
    # stores; round 3 had measured it no faster than the fp32 kernel with one load next to every store)
    split = lib().mode_deconv3d_split_bn_supported(Cin, Cout) == 1 and _deconv_split3d(Cin, Cout, (D, H, W))
    wp, reuse = _eval_wpack(bn, 'deconv3d_fwd_split_bn' if split else 'deconv3d_fwd_bn', w, lib().mode_conv3d_wpack_bytes(Cin, Cout) // 4, x.device)
    ay = _amax_for_consumer(y, False) if split else None
    tail = (ptr(wp), B, Cin, D, H, W, Cout, stream_of(x))
    with reuse:
      if split:
        _call('mode_deconv3d_fwd_split_bn_amax', ptr(x), ptr(w), ctypes.byref(e), ptr(y), _optr(ay), *tail)
      else:
        _call('mode_deconv3d_fwd_bn', ptr(x), ptr(w), ctypes.byref(e), ptr(y), *tail)
    _tag_amax(y, ay)
  return y


def conv2d_bn_eval(x, w, bn, dilation=1, add=None, relu=False):
  """Stride-1 3x3 convolution with padding = dilation (1 | 2) + eval BatchNorm (+ add) (+ ReLU)."""
  require_gpu(x, w)
  x, w = x.contiguous(), w.detach().contiguous()
  require_f32c(x, w)
  B, Ci, H, W = x.shape
  Co = w.shape[0]
  y = torch.empty((B, Co, H, W), dtype=x.dtype, device=x.device)
  e, keep = _epilogue(bn, add, relu, y)
  flops = 2 * y.numel() * Ci * 9
  with torch.cuda.device_of(x), profiling.region(_tag2d('conv2d_bn_eval', Ci, Co, dilation, H, W), 4 * (x.numel() + y.numel() + w.numel()), flops,
                                                 x.device):
    route = _conv2d_route(Ci, Co, H, W, dilation, 0, CONV2D_EVAL_F16)
    tag = {'f32': 'conv2d_fwd_bn', 'split': 'conv2d_fwd_split', 'split_f16': 'conv2d_fwd_split_f16_bn'}
    wp, reuse = _eval_wpack(bn, tag[route], w, lib().mode_conv2d_wpack_bytes(Ci, Co) // 4, x.device)
    ax = ay = None
    if route == 'split_f16':
      # two fp16 pieces (round 6): the input's maximum from its producer's tag (this kernel's own, in the residual blocks) or a pass
      ax, ay = _tagged_abs_max(x), torch.empty(BN_ABSMAX_FLOATS, dtype=torch.float32, device=x.device)
    tail = (ptr(wp), B, Ci, H, W, Co, dilation, stream_of(x))
    with reuse:
      if route == 'split_f16':
        _call('mode_conv2d_fwd_split_f16_bn', ptr(x), ptr(w), ptr(ax), ctypes.byref(e), ptr(y), ptr(ay), *tail)
      else:
        _call('mode_conv2d_fwd_split' if route == 'split' else 'mode_conv2d_fwd_bn', ptr(x), ptr(w), ctypes.byref(e), ptr(y), *tail)
    _tag_amax(y, ay)
  return y


def sphere_conv_bn_eval(x, pos, w, bn, stride, groups, add=None, relu=False, transposed=False):
  """Spherical (or integer-table) convolution + eval BatchNorm (+ add) (+ ReLU).  transposed: x, add and the result are in
  plane-transposed storage (B, C, W, H) -- only with a plannable table (sphere_t_supported)."""
  require_gpu(x, pos, w)
  x, w = x.contiguous(), w.detach().contiguous()
  require_f32c(x, pos, w)
  Co, _, Kh, Kw = w.shape
  if transposed:
    B, Ci, W, H = x.shape
    plan = sphere_plan(pos, Kh, Kw) if sphere_win_geometry(stride, Kh, Kw, True) else None
    if plan is None:
      raise RuntimeError('sphere_conv_bn_eval: plane-transposed storage needs a plannable sampling table')
  else:
    B, Ci, H, W = x.shape
    Ho, Wo = (H - 1) // stride[0] + 1, (W - 1) // stride[1] + 1  # (the table carries padding / dilation: 'same' geometry)
    route, plan = _sphere_fwd_route(pos, w, B, groups, stride, True, honour_switch=False)  # (inference never read SPHERE_FWD)
    if route == 'native_t':  # ERP-like table: NCHW storage is its transposed storage
      return sphere_conv_bn_eval(x, plan, w, bn, stride, groups, add, relu, transposed=True)
  flops = 2 * B * Co * H * W // (stride[0] * stride[1]) * w[0].numel()
  name = 'sphere_conv_bn_eval[%d->%d %dx%d]' % (Ci, Co, H, W) if profiling.ENABLED else 'sphere_conv_bn_eval'
  with torch.cuda.device_of(x), profiling.region(name, 4 * (2 * x.numel() + w.numel()), flops, x.device):
    if plan is None:
      return _sphere_gather_bn(x, pos, w, bn, stride, groups, add, relu, Ho, Wo)
    wp, reuse = _eval_wpack(bn, 'sphere_fwd_win g%d %dx%d' % (groups, H, W), w,
                            lib().mode_sphere_conv_win_wpack_bytes(Ci, Co, Kh, Kw, groups) // 4, w.device)
    # an NCHW caller: the windowed kernel on plane-transposed copies (the residual is transposed with it)
    xt = x if transposed else transpose_planes(x)
    yt = torch.empty((B, Co, W, H), dtype=x.dtype, device=x.device)
    e, keep = _epilogue(bn, add if transposed or add is None else transpose_planes(add.contiguous()), relu, yt)
    with reuse:
      _sphere_fwd_win(ptr(xt), pos, w, e, ptr(yt), wp, plan, B, Ci, H, W, Co, Kh, Kw, groups, 1, stream_of(x))
    return yt if transposed else transpose_planes(yt)


def _sphere_gather_bn(x, pos, w, bn, stride, groups, add, relu, Ho, Wo):
  """The general gather kernel with the folded-BatchNorm epilogue, under its packed-weight tag: the one launch of sphere_conv_bn_eval's
  gather route and of _tabled_bn, each inside its own profiling region."""
  B, Ci, H, W = x.shape
  Co, Cig, Kh, Kw = w.shape
  y = torch.empty((B, Co, Ho, Wo), dtype=x.dtype, device=x.device)
  e, keep = _epilogue(bn, add, relu, y)
  wp, reuse = _eval_wpack(bn, 'sphere_conv_fwd_bn g%d' % groups, w, lib().mode_sphere_conv_wpack_bytes(Cig * groups, Co, Kh, Kw, groups) // 4, w.device)
  with reuse:
    _call('mode_sphere_conv_fwd_bn', ptr(x), ptr(pos), ptr(w), ctypes.byref(e), ptr(y), ptr(wp), B, Ci, H, W, Co, Kh, Kw, stride[0], stride[1], Ho, Wo,
          groups, stream_of(x))
  return y


def conv2d_tabled_bn_eval(x, conv, bn, add=None, relu=False):
  """nn.Conv2d `conv` (anything but the stride-1 3x3 layers) + eval BatchNorm (+ add) (+ ReLU) on the gather-and-MAC kernel; a
  kernel with more than MAX_TAPS taps (the 7x7 stem) runs its first row bands plainly and the epilogue on the last."""
  x = x.contiguous()
  w = conv.weight.detach().contiguous()
  B, Ci, H, W = x.shape
  Co, _, kh, kw = w.shape
  stride, pad, dil = tuple(conv.stride), tuple(conv.padding), tuple(conv.dilation)
  Ho = (H + 2 * pad[0] - (dil[0] * (kh - 1) + 1)) // stride[0] + 1
  Wo = (W + 2 * pad[1] - (dil[1] * (kw - 1) + 1)) // stride[1] + 1
  bands = _row_bands(kh, kw)
  if len(bands) == 1:
    pos = conv2d_table(H, W, kh, kw, stride, pad, dil, x.device)
    y = _tabled_bn(x, pos, w, bn, stride, add, relu, Ho, Wo)
    return y
  # several bands (the 7x7 stem): every band would need the scale, and only the last one the shift -- not worth a second epilogue
  # form for one 3 -> 32 layer: the bands run plainly and one fused BatchNorm pass follows (a 67 MB tensor, once per image pair)
  y = torch.empty((B, Co, Ho, Wo), dtype=x.dtype, device=x.device)
  for r0, rows in bands:
    pos = conv2d_table(H, W, rows, kw, stride, pad, dil, x.device, r0)
    part = y if r0 == 0 else torch.empty_like(y)
    sphere_conv_fwd(x, pos, w[:, :, r0:r0 + rows].contiguous(), part, stride, 1)
    if r0:
      y += part
  return bn_eval(y, add, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, relu)


def _tabled_bn(x, pos, w, bn, stride, add, relu, Ho, Wo):
  B, Ci, H, W = x.shape
  Co = w.shape[0]
  flops = 2 * B * Co * Ho * Wo * w[0].numel()
  name = 'sphere_conv_bn_eval[%d->%d %dx%d]' % (Ci, Co, H, W) if profiling.ENABLED else 'sphere_conv_bn_eval'
  with torch.cuda.device_of(x), profiling.region(name, 4 * (x.numel() + B * Co * Ho * Wo + w.numel()), flops, x.device):
    return _sphere_gather_bn(x, pos, w, bn, stride, 1, add, relu, Ho, Wo)


def cost_conv_bn_eval(ref, tgt, weight, d4, bn, relu=True):
  """relu?(bn(conv3d(cost_volume(ref, tgt, d4), weight))) in eval mode, without the volume (cost_conv + folded BatchNorm)."""
  C = ref.shape[1]
  R, T = _tap_products(ref, weight[:, :C]), _tap_products(tgt, weight[:, C:])
  require_f32c(R, T)
  B, C9, H, W = R.shape
  Co = C9 // 9
  out = torch.empty((B, Co, d4, H, W), dtype=R.dtype, device=R.device)
  e, keep = _epilogue(bn, None, relu, out)
  with torch.cuda.device_of(R), profiling.region('cost_conv_assemble_fwd', 4 * (R.numel() + T.numel() + out.numel()), 0, R.device):
    ay = _amax_for_consumer(out, False)
    _call('mode_cost_conv_assemble_fwd_bn_amax', ptr(R), ptr(T), ctypes.byref(e), ptr(out), _optr(ay), B, Co, d4, H, W, stream_of(R))
    _tag_amax(out, ay)
  return out
