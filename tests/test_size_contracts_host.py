"""Host tier (no GPU): the 32-bit size contracts of the split-operand convolution kernels (csrc/size_contracts.h).

The kernels stage their operands with buffer loads: a descriptor of `bytes` bytes, a 32-bit lane offset, and a SENTINEL offset for a
position in the zero padding, which must read as zero.  That is right only while
    largest valid offset < descriptor bytes < smallest sentinel, and every sentinel sum < 2^32,
as the 32-bit quantities the kernels compute.  The two ABI predicates mode_conv3d_split_shape_supported /
mode_conv2d_split_shape_supported are the one host-side source of these limits; this file probes them at the last shape inside and
the first shape beyond every limit and compares them with a restatement of each kernel's address arithmetic in plain Python
integers (`_contract_*` below: written from the kernels' expressions -- file and lambda named at each -- not from the predicates).

`bytes < sentinel` is asserted STRICTLY, as common.h states the contract ("bytes < 2^31 is the caller's contract"): the shapes that
must be refused -- 1024 x 128 x 512 (32 DHW = 2^31), 256 x 128 x 512 at 16 -> 16 (128 DHW = 2^31), 2048 x 4096 (128 HW = 2^30) -- sit
exactly ON the sentinel, where a `<=` would accept them.

No test here hands a made-up non-null address to a launching entry: this tier also runs on GPU machines.  Refusals are checked
through the entries with NULL tensors only, where sizes are validated before pointers: beyond a limit MODE_ERR_UNSUPPORTED, inside it
MODE_ERR_BAD_ARG for the null pointer -- nothing is launched either way."""
import pytest

import mode_hip
from mode_hip import functional as HF

OK, BAD_ARG, UNSUPPORTED = 0, -1, -2
U32 = 1 << 32
KBUF_OOB = 1 << 31   # common.h: kBufOOB
KHALF_OOB = 1 << 30  # conv2d_split_wgrad.hip: kHalfOOB


@pytest.fixture(scope='module')
def lib():
  return mode_hip.lib()


def _holds(c):
  """The contract of a restatement `c`: valid offsets inside the descriptor, the descriptor below every sentinel, no sum wraps, and the
  element count of the sample the kernel indexes (`max_index`: one past its last element, the largest value its 32-bit index or byte
  offset arithmetic forms) inside that arithmetic's range."""
  return [c['max_valid'] < c['bytes'], c['max_valid'] < c['min_sentinel'], c['bytes'] < c['min_sentinel'], c['max_sentinel'] < U32,
          c['max_index'] < c['index_limit']]


# ------------------------------------------------------------------------------------------------ restatements of the kernels' arithmetic
def _contract_s1(K, rows, D, H, W):
  """conv3d_split.hip (stage_begin / stage_load; conv3d_split_s2.hip and conv3d_split_deconv.hip stage alike): descriptor
  (unsigned)DHW * 32u over a chunk of 8 channel planes; lane offset (st_base + poff) * 4 of a voxel; channel c the scalar offset
  c * DHW * 4; padding -> kBufOOB.  Epilogue: element index o * DHW + voxel inside a sample of `rows` channels (int)."""
  DHW = D * H * W
  return dict(bytes=32 * DHW, max_valid=4 * (DHW - 1) + 7 * DHW * 4, min_sentinel=KBUF_OOB, max_sentinel=KBUF_OOB + 7 * DHW * 4,
              max_index=rows * DHW, index_limit=1 << 31)


def _contract_s2_fwd(K, rows, D, H, W):
  """conv3d_split_s2.hip: the same descriptor over the INPUT volume; its epilogue indexes the output with 64-bit offsets (oDHW is a
  long long there): no element limit."""
  c = _contract_s1(K, rows, D, H, W)
  c.update(max_index=0)
  return c


def _contract_deconv(K, Co, d, h, w):
  """conv3d_split_deconv.hip: descriptor over the LOW-resolution input d x h x w of K channels; the epilogue's own offsets are 64-bit, and the entry
  keeps the sample limit it had before the buffer loads -- an output sample of 8 dhw voxels in max(Co, 8) channels below 2^31 elements --
  which is also what the fp32 kernel behind the fallback takes (mode_deconv3d_fwd: Cout * 8 dhw < 2^31)."""
  dhw = d * h * w
  return dict(bytes=32 * dhw, max_valid=4 * (dhw - 1) + 7 * dhw * 4, min_sentinel=KBUF_OOB, max_sentinel=KBUF_OOB + 7 * dhw * 4,
              max_index=8 * dhw * max(Co, 8), index_limit=1 << 31)


def _contract_wgrad3d(Ci, Co, D, H, W):
  """conv3d_split_wgrad.hip (unit_begin / load_x / load_g): block_bytes = 128u * DHW -- 32 channel planes WHATEVER the channel count;
  lane offset 4 * (c * DHW + row * W + col) (+ 4 for the pair's second column), c < min(C, 32); the plane z the scalar offset
  4 * z * HW; padding and channels beyond the layer's -> kBufOOB.  Element offsets of a sample: max(Ci, Co) * DHW in 32-bit ints with
  the 4x byte scaling applied to them (< 2^29)."""
  DHW, HW = D * H * W, H * W
  cmax = min(max(Ci, Co), 32) - 1
  return dict(bytes=128 * DHW, max_valid=4 * (cmax * DHW + (H - 1) * W + (W - 1)) + 4 * (D - 1) * HW, min_sentinel=KBUF_OOB,
              max_sentinel=KBUF_OOB + 4 * (D - 1) * HW, max_index=max(Ci, Co) * DHW, index_limit=1 << 29)


def _contract_wgrad3d_s2(Ci, Co, D, H, W):
  """conv3d_split_wgrad_s2.hip (no buffer loads): unsigned BYTE offsets 4 * (c * DHW + ...) inside a 32-channel block of x and
  4 * (o * oDHW + ...) inside a 64-channel block of gy, added to the plane's -- both must stay below 2^31 (the kernel's 4u * (unsigned)
  products of ints)."""
  DHW, oDHW = D * H * W, (D // 2) * (H // 2) * (W // 2)
  return dict(bytes=1, max_valid=0, min_sentinel=2, max_sentinel=2,  # (no descriptor)
              max_index=max(min(Ci, 32) * DHW, min(Co, 64) * oDHW), index_limit=1 << 29)


def _contract_c2d(K, rows, H, W, dil):
  """conv2d_split.hip (stage_begin / stage_load): descriptor (unsigned)HW * 64u over a chunk of 16 channel planes, lane offset
  (st_base + poff) * 4, channel c the scalar offset c * HW * 4, padding -> kBufOOB; int element offsets of a sample (< 2^29 with the
  byte scaling)."""
  HW = H * W
  return dict(bytes=64 * HW, max_valid=4 * (HW - 1) + 15 * HW * 4, min_sentinel=KBUF_OOB, max_sentinel=KBUF_OOB + 15 * HW * 4,
              max_index=max(K, rows) * HW, index_limit=1 << 29)


def _contract_wgrad2d(Ci, Co, H, W, dil):
  """conv2d_split_wgrad.hip (unit_begin / load_x / load_g): block_bytes = 128u * HW; the lane offset is column part + row part:
    column part  4 * (c * HW + j * W + col) (+ 4), j = 0..3 the row inside the staged group of four, or kHalfOOB;
    row part     4 * r0 * W for the group's first row r0 when r0 + j is a row of the image, or kHalfOOB;
  x groups start at r0 = h - dil (prologue: h_first - DIL; steady state: h0 - DIL + 8), so r0 >= -dil and the row part is NEGATIVE
  for the top halo while rows r0 + j >= 0 of that group are valid; gy groups at r0 >= 0."""
  HW = H * W
  cmax = min(max(Ci, Co), 32) - 1
  r0_min = -dil                                   # a valid row of the first x group: j = dil
  r0_max = H - 1                                  # j = 0 on the last row
  col_max = 4 * (cmax * HW + 3 * W + (W - 1)) + 4  # the largest column part, second column of the pair
  sentinels = [KHALF_OOB + 4 * r0_min * W,        # invalid column, valid row of the top halo group
               KHALF_OOB + 4 * r0_max * W,        # invalid column, last valid row
               KHALF_OOB + 0,                     # valid column 0 of channel 0, invalid row
               KHALF_OOB + col_max,               # valid column, invalid row
               KHALF_OOB + KHALF_OOB]             # both invalid
  return dict(bytes=128 * HW, max_valid=4 * (cmax * HW + (H - 1) * W + (W - 1)), min_sentinel=min(sentinels), max_sentinel=max(sentinels),
              max_index=max(Ci, Co) * HW, index_limit=1 << 29)


# ------------------------------------------------------------------------------------------------ probes: (inside, beyond) per limit
# 3-D: (Ci, Co, stride, which, restatement of (Ci, Co, D, H, W), [(inside, beyond), ...]).  Channel counts at the smallest and the
# largest supported value of each family; boundaries of a limit are walked with 1 x 1 x N volumes (exact) and with the shapes of the
# issue's table.
def _s1(which):
  def f(Ci, Co, D, H, W):
    return _contract_s1(Co, Ci, D, H, W) if which == 1 else _contract_s1(Ci, Co, D, H, W)
  return f


def _s2_bwd_data(Ci, Co, D, H, W):  # the transposed kernel on gy (Co channels at half the volume) -> gx (Ci channels)
  return _contract_deconv(Co, Ci, D // 2, H // 2, W // 2)


P26, P24 = 1 << 26, 1 << 24
PROBES_3D = [
    # stride-1 forward / input gradient: 32 DHW < 2^31 (hole 1), and rows * DHW < 2^31 at 64 rows
    (8, 8, 1, 0, _s1(0), [((1023, 128, 512), (1024, 128, 512)), ((1, 1, P26 - 1), (1, 1, P26))]),
    (8, 2, 1, 0, _s1(0), [((1, 1, P26 - 1), (1, 1, P26))]),
    (64, 64, 1, 0, _s1(0), [((511, 128, 512), (512, 128, 512)), ((1, 1, (1 << 25) - 1), (1, 1, 1 << 25))]),
    (8, 8, 1, 1, _s1(1), [((1023, 128, 512), (1024, 128, 512)), ((1, 1, P26 - 1), (1, 1, P26))]),
    (2, 8, 1, 1, _s1(1), [((1, 1, P26 - 1), (1, 1, P26))]),
    (64, 64, 1, 1, _s1(1), [((1, 1, (1 << 25) - 1), (1, 1, 1 << 25))]),
    # stride-1 weight gradient: 128 DHW < 2^31 whatever the channel count (hole 2); max(Ci, Co) * DHW < 2^29 takes over above 32 channels
    (16, 16, 1, 2, _contract_wgrad3d, [((255, 128, 512), (256, 128, 512)), ((1, 1, P24 - 1), (1, 1, P24))]),
    (1, 2, 1, 2, _contract_wgrad3d, [((1, 1, P24 - 1), (1, 1, P24))]),
    (32, 32, 1, 2, _contract_wgrad3d, [((1, 1, P24 - 1), (1, 1, P24))]),
    (64, 64, 1, 2, _contract_wgrad3d, [((1, 1, (1 << 23) - 1), (1, 1, 1 << 23))]),
    # stride-2 forward (33..64 output channels): 32 DHW < 2^31 of the input volume
    (8, 33, 2, 0, _contract_s2_fwd, [((1023, 128, 512), (1024, 128, 512)), ((1, 1, P26 - 1), (1, 1, P26))]),
    (64, 64, 2, 0, _contract_s2_fwd, [((1, 1, P26 - 1), (1, 1, P26))]),
    # stride-2 input gradient = the transposed kernel on the half-resolution gradient: 8 * dhw * max(Ci, 8) < 2^31
    (8, 8, 2, 1, _s2_bwd_data, [((2, 2, (1 << 26) - 2), (2, 2, 1 << 26))]),
    (2, 8, 2, 1, _s2_bwd_data, [((2, 2, (1 << 26) - 2), (2, 2, 1 << 26))]),
    (64, 64, 2, 1, _s2_bwd_data, [((2, 2, (1 << 23) - 2), (2, 2, 1 << 23))]),
    # stride-2 weight gradient (x in blocks of 32 channels, gy of 64): min(Ci, 32) * DHW < 2^29
    (32, 64, 2, 2, _contract_wgrad3d_s2, [((2, 2, (1 << 22) - 8), (2, 2, 1 << 22))]),
    (64, 128, 2, 2, _contract_wgrad3d_s2, [((2, 2, (1 << 22) - 8), (2, 2, 1 << 22))]),
]


@pytest.mark.parametrize('Ci,Co,stride,which,restate,pairs', PROBES_3D, ids=lambda v: None if callable(v) or isinstance(v, list) else str(v))
def test_conv3d_predicate_sits_on_the_kernels_own_limits(lib, Ci, Co, stride, which, restate, pairs):
  assert lib.mode_conv3d_split_supported(Ci, Co, stride, which) == 1, 'the probe holds the channel counts at supported values'
  for inside, beyond in pairs:
    c_in, c_out = restate(Ci, Co, *inside), restate(Ci, Co, *beyond)
    print('%d->%d s%d which %d: inside %s %s | beyond %s %s' % (Ci, Co, stride, which, inside, c_in, beyond, c_out))
    assert lib.mode_conv3d_split_shape_supported(Ci, Co, *inside, stride, which) == 1, inside
    assert all(_holds(c_in)), (inside, c_in)
    assert lib.mode_conv3d_split_shape_supported(Ci, Co, *beyond, stride, which) == 0, beyond
    assert not all(_holds(c_out)), (beyond, c_out)


def test_transposed_convolution_asks_as_the_stride2_input_gradient(lib):
  """mode_deconv3d_fwd_split (Cin, d, h, w) -> (Cout, 2d, 2h, 2w) is the input gradient of the stride-2 convolution Cout -> Cin over the
  doubled volume: 8 * dhw * max(Cout, 8) < 2^31 (the descriptor's 32 dhw < 2^31 is implied)."""
  for cin, cout, n_in, n_out in ((8, 2, (1 << 25) - 1, 1 << 25), (64, 64, (1 << 22) - 1, 1 << 22), (8, 32, (1 << 23) - 1, 1 << 23)):
    assert lib.mode_deconv3d_split_supported(cin, cout) == 1
    assert lib.mode_conv3d_split_shape_supported(cout, cin, 2, 2, 2 * n_in, 2, 1) == 1 and all(_holds(_contract_deconv(cin, cout, 1, 1, n_in)))
    assert lib.mode_conv3d_split_shape_supported(cout, cin, 2, 2, 2 * n_out, 2, 1) == 0 and not all(_holds(_contract_deconv(cin, cout, 1, 1, n_out)))
    HF.set_conv_arith('bf16x6')
    assert HF._deconv_split3d(cin, cout, (1, 1, n_in)) and not HF._deconv_split3d(cin, cout, (1, 1, n_out))


def test_stride2_entries_keep_their_parity_requirements_in_the_predicate(lib):
  """Even D, H, W for the stride-2 input gradient; even D, H and W % 8 == 0 for the stride-2 weight gradient: part of `the shape is
  supported`, so that a dispatcher asks one question."""
  assert lib.mode_conv3d_split_shape_supported(64, 64, 8, 8, 8, 2, 1) == 1
  for vol in ((7, 8, 8), (8, 7, 8), (8, 8, 7)):
    assert lib.mode_conv3d_split_shape_supported(64, 64, *vol, 2, 1) == 0
  assert lib.mode_conv3d_split_shape_supported(32, 64, 8, 8, 8, 2, 2) == 1
  for vol in ((7, 8, 8), (8, 7, 8), (8, 8, 12)):
    assert lib.mode_conv3d_split_shape_supported(32, 64, *vol, 2, 2) == 0
  assert lib.mode_conv3d_split_shape_supported(32, 64, 7, 7, 7, 2, 0) == 1  # (the forward takes odd volumes)


def test_unsupported_channels_and_degenerate_arguments_are_refused(lib):
  p3, p2 = lib.mode_conv3d_split_shape_supported, lib.mode_conv2d_split_shape_supported
  assert p3(12, 32, 4, 4, 4, 1, 0) == 0 and p3(32, 96, 4, 4, 4, 1, 0) == 0 and p3(32, 1, 4, 4, 4, 1, 2) == 0
  assert p3(32, 32, 4, 4, 4, 2, 0) == 0 and p3(32, 32, 4, 4, 4, 3, 0) == 0 and p3(32, 32, 4, 4, 4, 1, 3) == 0
  assert p3(32, 32, 0, 4, 4, 1, 0) == 0 and p3(32, 32, 4, -1, 4, 1, 0) == 0 and p3(0, 32, 4, 4, 4, 1, 0) == 0
  assert p2(12, 32, 8, 8, 1, 0) == 0 and p2(32, 12, 8, 8, 1, 1) == 0 and p2(32, 32, 8, 8, 3, 0) == 0 and p2(32, 32, 8, 8, 1, 3) == 0
  assert p2(12, 5, 8, 8, 2, 2) == 1 and p2(32, 32, 0, 8, 1, 2) == 0 and p2(0, 32, 8, 8, 1, 2) == 0
  # the model's own layers, at the benchmark's sizes: far inside
  assert p3(32, 32, 48, 256, 128, 1, 0) == 1 and p3(64, 64, 24, 128, 64, 1, 2) == 1 and p3(32, 64, 48, 256, 128, 2, 0) == 1
  assert p3(32, 64, 48, 256, 128, 2, 2) == 1 and p3(64, 64, 24, 128, 64, 2, 1) == 1 and p2(32, 32, 1024, 512, 2, 2) == 1


# 2-D: (Ci, Co, dilation, which, restatement, [(inside, beyond) as (H, W)]).
def _c2d(which):
  def f(Ci, Co, H, W, dil):
    return _contract_c2d(Co, Ci, H, W, dil) if which == 1 else _contract_c2d(Ci, Co, H, W, dil)
  return f


def _top_halo_pair(dil):
  """One-row images around 128 W + 4 dil W = 2^30: the shapes at which ONLY the negative row part of the top halo decides (128 HW itself
  is still below 2^30)."""
  n = -(-(1 << 30) // (128 + 4 * dil))  # the first W with (128 + 4 dil) W >= 2^30
  assert 128 * n < (1 << 30)
  return ((1, n - 1), (1, n))


PROBES_2D = [(ci, co, dil, which, _c2d(which), pairs)
             for which in (0, 1) for dil in (1, 2)
             for ci, co, pairs in ((16, 16, [((1, (1 << 25) - 1), (1, 1 << 25)), ((4095, 8192), (4096, 8192))]),
                                   (16, 2, [((1, (1 << 25) - 1), (1, 1 << 25))]) if which == 0 else (2, 16, [((1, (1 << 25) - 1), (1, 1 << 25))]),
                                   (512, 512, [((1, (1 << 20) - 1), (1, 1 << 20))]))]
PROBES_2D += [(ci, co, dil, 2, _contract_wgrad2d, [((2040, 4096), (2048, 4096)), ((2047, 4096), (2048, 4096)), ((2040, 4096), (2056, 4096)),
                                                   _top_halo_pair(dil)])
              for dil in (1, 2) for ci, co in ((32, 32), (16, 16), (1, 1), (32, 5))]
PROBES_2D += [(c, c, dil, 2, _contract_wgrad2d, [((1, (1 << 29) // c - 1), (1, (1 << 29) // c))])  # (max(Ci, Co) * HW < 2^29 comes first)
              for dil in (1, 2) for c in (128, 512)]


@pytest.mark.parametrize('Ci,Co,dil,which,restate,pairs', PROBES_2D, ids=lambda v: None if callable(v) or isinstance(v, list) else str(v))
def test_conv2d_predicate_sits_on_the_kernels_own_limits(lib, Ci, Co, dil, which, restate, pairs):
  if which != 2:
    assert lib.mode_conv2d_split_supported(Ci, Co, dil, which) == 1, 'the probe holds the channel counts at supported values'
  for inside, beyond in pairs:
    c_in, c_out = restate(Ci, Co, *inside, dil), restate(Ci, Co, *beyond, dil)
    print('%d->%d d%d which %d: inside %s %s | beyond %s %s' % (Ci, Co, dil, which, inside, c_in, beyond, c_out))
    assert lib.mode_conv2d_split_shape_supported(Ci, Co, *inside, dil, which) == 1, inside
    assert all(_holds(c_in)), (inside, c_in)
    assert lib.mode_conv2d_split_shape_supported(Ci, Co, *beyond, dil, which) == 0, beyond
    assert not all(_holds(c_out)), (beyond, c_out)


def test_the_top_halo_marker_is_what_refuses_the_last_images(lib):
  """Hole 3's second detail: at the one-row boundary image the descriptor alone is still below kHalfOOB -- the negative row part of the
  top halo is the smallest sentinel, and it lies inside the block."""
  for dil in (1, 2):
    (h, w), (h2, w2) = _top_halo_pair(dil)
    c = _contract_wgrad2d(32, 32, h2, w2, dil)
    assert c['bytes'] < KHALF_OOB and c['min_sentinel'] <= c['bytes'] and c['min_sentinel'] == KHALF_OOB - 4 * dil * w2
    assert lib.mode_conv2d_split_shape_supported(32, 32, h2, w2, dil, 2) == 0 and lib.mode_conv2d_split_shape_supported(32, 32, h, w, dil, 2) == 1


# ------------------------------------------------------------------------------------------------ the entries ask the same predicate
N = None


def _entries_3d(lib, Ci, Co, vol, stride, which):
  """(name, return code) of every launching split entry of (stride, which), called with NULL tensors, B = 1: sizes are validated before
  pointers, so nothing can be launched."""
  D, H, W = vol
  out = []
  if stride == 1 and which == 0:
    out.append(('mode_conv3d_fwd_split', lib.mode_conv3d_fwd_split(N, N, N, N, N, 1, Ci, D, H, W, Co, N)))
    out.append(('mode_conv3d_fwd_split_stats', lib.mode_conv3d_fwd_split_stats(N, N, N, N, N, 1, Ci, D, H, W, Co, N)))
    out.append(('mode_conv3d_fwd_split_f16', lib.mode_conv3d_fwd_split_f16(N, N, N, N, N, N, 1, Ci, D, H, W, Co, N)))
    out.append(('mode_conv3d_fwd_split_f16_bn', lib.mode_conv3d_fwd_split_f16_bn(N, N, N, N, N, N, N, 1, Ci, D, H, W, Co, N)))
  elif stride == 1 and which == 1:
    out.append(('mode_conv3d_bwd_data_split', lib.mode_conv3d_bwd_data_split(N, N, N, N, 1, Ci, D, H, W, Co, N)))
    out.append(('mode_conv3d_bwd_data_split_acc', lib.mode_conv3d_bwd_data_split_acc(N, N, N, N, N, 1, Ci, D, H, W, Co, 1, N)))
    out.append(('mode_conv3d_bwd_data_split_f16', lib.mode_conv3d_bwd_data_split_f16(N, N, N, N, N, N, N, 1, Ci, D, H, W, Co, N)))
  elif stride == 1:
    out.append(('mode_conv3d_bwd_weight_split', lib.mode_conv3d_bwd_weight_split(N, N, N, N, 1, Ci, D, H, W, Co, 0, N)))
  elif which == 0:
    out.append(('mode_conv3d_fwd_s2_split', lib.mode_conv3d_fwd_s2_split(N, N, N, N, N, 1, Ci, D, H, W, Co, N)))
    out.append(('mode_conv3d_fwd_s2_split_amax', lib.mode_conv3d_fwd_s2_split_amax(N, N, N, N, N, N, 1, Ci, D, H, W, Co, N)))
  elif which == 1:
    out.append(('mode_conv3d_bwd_data_s2_split', lib.mode_conv3d_bwd_data_s2_split(N, N, N, N, 1, Ci, D, H, W, Co, N)))
    out.append(('mode_conv3d_bwd_data_split_acc', lib.mode_conv3d_bwd_data_split_acc(N, N, N, N, N, 1, Ci, D, H, W, Co, 2, N)))
  else:
    out.append(('mode_conv3d_bwd_weight_s2_split', lib.mode_conv3d_bwd_weight_s2_split(N, N, N, N, 1, Ci, D, H, W, Co, 0, N)))
  return out


@pytest.mark.parametrize('Ci,Co,stride,which,restate,pairs', PROBES_3D, ids=lambda v: None if callable(v) or isinstance(v, list) else str(v))
def test_conv3d_entries_refuse_beyond_the_limit_before_they_look_at_a_pointer(lib, Ci, Co, stride, which, restate, pairs):
  for inside, beyond in pairs:
    for name, rc in _entries_3d(lib, Ci, Co, beyond, stride, which):
      assert rc == UNSUPPORTED, (name, beyond, rc, lib.mode_last_error())
    # The ABI's own sample limit -- max(C, 8) * D * H * W < 2^31 on the entry's volume, in front of everything in every 3-D entry -- ends
    # before some of the kernels' limits do (the stride-2 forward's 33+ output channels, the stride-2 input gradient): there the entry
    # answers MODE_ERR_UNSUPPORTED on both sides and only the predicate shows where the kernel's own limit is.
    abi_ok = max(Ci, Co, 8) * inside[0] * inside[1] * inside[2] < 2**31
    for name, rc in _entries_3d(lib, Ci, Co, inside, stride, which):
      assert rc == (BAD_ARG if abi_ok else UNSUPPORTED), (name, inside, rc, lib.mode_last_error())


def test_the_three_holes_through_their_entries(lib):
  """The calls of the issue: accepted by validation before this change, and the kernel then read garbage for the padding, or zeros
  for everything.  Now MODE_ERR_UNSUPPORTED; the neighbouring shape inside the limit still reaches the pointer check."""
  assert lib.mode_conv3d_fwd_split(N, N, N, N, N, 1, 8, 1024, 128, 512, 8, N) == UNSUPPORTED
  assert lib.mode_conv3d_fwd_split(N, N, N, N, N, 1, 8, 1023, 128, 512, 8, N) == BAD_ARG
  assert lib.mode_conv3d_bwd_weight_split(N, N, N, N, 1, 16, 256, 128, 512, 16, 0, N) == UNSUPPORTED
  assert lib.mode_conv3d_bwd_weight_split(N, N, N, N, 1, 16, 255, 128, 512, 16, 0, N) == BAD_ARG
  for dil in (1, 2):
    for c in (32, 16):
      assert lib.mode_conv2d_bwd_weight_split(N, N, N, N, 1, c, 2056, 4096, c, dil, 0, N) == UNSUPPORTED
      assert lib.mode_conv2d_bwd_weight_split(N, N, N, N, 1, c, 2048, 4096, c, dil, 0, N) == UNSUPPORTED
      assert lib.mode_conv2d_bwd_weight_split(N, N, N, N, 1, c, 2040, 4096, c, dil, 0, N) == BAD_ARG
  # the transposed entries: (Cin, d, h, w) -> (Cout, 2d, 2h, 2w)
  assert lib.mode_deconv3d_fwd_split(N, N, N, N, 1, 8, 1, 1, 1 << 25, 2, N) == UNSUPPORTED
  assert lib.mode_deconv3d_fwd_split(N, N, N, N, 1, 8, 1, 1, (1 << 25) - 1, 2, N) == BAD_ARG
  # 2-D forward / input gradient
  assert lib.mode_conv2d_fwd_split(N, N, N, N, N, 1, 16, 1, 1 << 25, 16, 1, N) == UNSUPPORTED
  assert lib.mode_conv2d_fwd_split(N, N, N, N, N, 1, 16, 1, (1 << 25) - 1, 16, 1, N) == BAD_ARG
  assert lib.mode_conv2d_bwd_data_split(N, N, N, N, 1, 16, 1, 1 << 25, 16, 2, N) == UNSUPPORTED
  assert lib.mode_conv2d_bwd_data_split(N, N, N, N, 1, 16, 1, (1 << 25) - 1, 16, 2, N) == BAD_ARG


# ------------------------------------------------------------------------------------------------ the Python dispatchers ask it too
class _Shape(object):
  def __init__(self, *shape):
    self.shape = tuple(shape)


def test_python_dispatch_helpers_agree_with_the_predicates(lib):
  try:
    for (Ci, Co, stride, which, _, pairs) in PROBES_3D:
      for inside, beyond in pairs:
        HF.set_conv_arith('bf16x6')
        assert HF._split3d(Ci, Co, stride, which, inside) is True and HF._split3d(Ci, Co, stride, which, beyond) is False
        assert HF._split3d(Ci, Co, stride, which) is True, 'without a volume: the channel counts alone'
        HF.set_conv_arith('f32')
        assert HF._split3d(Ci, Co, stride, which, inside) is False
    HF.set_conv_arith('bf16x6')
    assert HF.conv3d_s1_f16(8, 8, 0, (1023, 128, 512)) == HF.CONV3D_S1_F16 and not HF.conv3d_s1_f16(8, 8, 0, (1024, 128, 512))
    # conv2d_bwd_weight has a right kernel at the panorama size -- the fp32 one -- and none beyond max(Ci, Co) * HW < 2^29
    for arith in ('bf16x6', 'f32'):
      HF.set_conv_arith(arith)
      assert HF.conv2d_wgrad_supported(_Shape(1, 32, 2040, 4096), _Shape(32, 32, 3, 3))
      assert HF.conv2d_wgrad_supported(_Shape(1, 32, 2048, 4096), _Shape(32, 32, 3, 3))
      assert HF.conv2d_wgrad_supported(_Shape(1, 32, 4095, 4096), _Shape(32, 32, 3, 3))
      assert not HF.conv2d_wgrad_supported(_Shape(1, 32, 4096, 4096), _Shape(32, 32, 3, 3))
  finally:
    HF.set_conv_arith('bf16x6')


def test_both_predicates_are_registered_host_only_names():
  """`_supported` in the names: the poisoning proxy and the guard-band ledger treat them as host-only without edits."""
  for name in ('mode_conv3d_split_shape_supported', 'mode_conv2d_split_shape_supported'):
    assert name in mode_hip.SIGNATURES and '_supported' in name
  assert len(mode_hip.SIGNATURES['mode_conv3d_split_shape_supported'][1]) == 7
  assert len(mode_hip.SIGNATURES['mode_conv2d_split_shape_supported'][1]) == 6
