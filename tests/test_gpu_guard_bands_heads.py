"""Guard bands AND float64 for every compiled form of the two heads of the 3-D stage: the soft-argmin head (csrc/head.hip) at the
instantiated depths no gradient test reached (D4 = 8, 16, 64) and in both forms of its fast backward, and the fused classifier head's
backward (csrc/classif_head.hip) in every tile width of its 16-byte kernels, ragged tiles and fewer than 32 channels included.

As tests/test_gpu_guard_bands_conf_grad.py: the cases are registered in the operator table of tests/test_gpu_guard_bands.py
(test_gpu_guard_bands.CASES, through its own case() helper) when this module is imported, and run here through
test_gpu_guard_bands.run_case: the declared entries launched, guards intact under both fills, outputs bit-equal between the fills
(every element written) and finite, and the builder's verify() against a float64 CPU reference -- b_head / b_head_loss (oracle/mode_ref.py
under autograd, tests/conf_grad_ref.py) and b_classif (test_gpu_classif._reference, torch's own CPU operators in float64) with their
standing bounds.  No kernel is compared only with another kernel of this library.

THE SOFT-ARGMIN HEAD.  Shapes (B, D4, H4, W4), output 4 x in every dimension, logits _rand(shape, 61, 3.0), upstream gradients of seeds
62 and 63.  MODE_HEAD_FAST_D4 instantiates every fast kernel for D4 = 4, 8, 12, 16, 48, 64; node indices and lerp weights are the
compile-time HeadConst<D4>, different code for every D4.  The backward's routing (head_bwd_run) takes one of two fast forms:

  rows    pixrows_fits (= HF.head_loss_supported, asserted true by every such case): head_bwd_pixrows_kernel<D4, LOSS, CONF>, one block per
          image row, the node gradients through LDS HR_KC = 16 at a time, then head_bwd_cols_kernel
  pixels  W = 28 over W4 = 7: 64 threads are no whole number of node rows (HF.head_loss_supported asserted false):
          head_bwd_pix_fast_kernel<D4, CONF>, then head_bwd_rows_kernel and head_bwd_cols_kernel

  case                     mode_head_fwd                  mode_head_bwd            mode_head_bwd_conf
  head_rows   (1, 8,3, 8)  fwd_fast<8, false / true>      pixrows<8, false, false>   pixrows<8, false, true>     one partial LDS pass
  head_rows   (1,16,3, 8)  fwd_fast<16, .>                pixrows<16, false, false>  pixrows<16, false, true>    exactly one full pass
  head_rows   (1,64,2, 8)  fwd_fast<64, .> (conf: 64 KB   pix_fast<64, false> + rows  pix_fast<64, true> + rows    the row kernel fits, and is
  head_rows   (2,64,3,16)  of dynamic LDS)                + columns                   + columns                   not taken (below)
  head_pixels (1, 8,3, 7)  fwd_fast<8, .>                 pix_fast<8, false> + r + c  pix_fast<8, true> + r + c
  head_pixels (1,16,2, 7)  fwd_fast<16, .>                pix_fast<16, false> ...     pix_fast<16, true> ...
  head_pixels (1,48,2, 7)  fwd_fast<48, .>                pix_fast<48, false> ...     pix_fast<48, true> ...      the network's own D4
  head_pixels (1,64,2, 7)  fwd_fast<64, .>                pix_fast<64, false> ...     pix_fast<64, true> ...
  head_loss_rows (1, 8,4,8), (1,16,4,8), (1,64,3,8): mode_head_bwd_loss = pixrows<D4, true, false> (+ mode_smooth_l1_masked); at
                                                      D4 = 64 four LDS passes of the kernel that fills the register file and spills

The confidence backward at D4 = 64 takes the SECOND form at every shape, also where the row kernel fits: kPixrowsConfMaxD4 = 48
(pixrows<64, ., true> is not compiled; the plain one already fills the register file).  These cases found mode_head_bwd on the row
kernel there: two different kernels, whose shared arithmetic the compiler rounds independently, and "mode_head_bwd_conf with gconf == 0
has the bits of mode_head_bwd" (include/mode_hip.h) was off by a few ulp at (1, 64, 2, 8) and (2, 64, 3, 16).  mode_head_bwd now takes
the second form at D4 = 64 too; the row kernel of that depth is reached by mode_head_bwd_loss alone.
head_border_*: the same checks on logits with +14 on node 0 over the first W4 // 3 columns and on node D4 - 1 over the last W4 // 3
(test_gpu_guard_bands._head_reference): at least 5 % of the float64 predictions round to 0 and 5 % to D - 1, the reference confidence
exceeds 1.5 -- window indices that count twice, at depths where the window's nodes are the run-time src_index next to HeadConst<D4>.

THE CLASSIFIER HEAD.  Shapes (B, C, (D, H, W)); the inputs of test_fused_classifier_head_small_and_ragged; both CONV_ARITH values (f32:
classif_bwd_apply2_kernel<TC, false>; bf16x6: <TC, true>, and the plain twin through PlainTwins bit for bit).  Every case has W % 4 == 0
and 16-byte aligned tensors, so mode_classif_train_bwd runs classif_bww2_kernel<TC> and classif_bwd_apply2_kernel<TC, AMAX>, TC =
tile_cols(W): 128 for W > 64, 64 for W > 32, 32 otherwise (the table next to CLASSIF below).  None of these cases has an element within
1e-5 of the ReLU threshold in float64 (asserted): every element of gy is compared.
classif_off_grid: (1, 32, (3, 5, 40)) with the backward's y one element into a larger buffer -- W % 4 == 0 but the base 4 bytes off
the 16-byte grid, so mode_classif_train_bwd takes classif_bww_kernel and classif_bwd_apply_kernel (the dword forms), under the same
bounds.  The forward refuses such a view (its statistics pass reads 16-byte pieces: "unaligned buffer", an error and no fall-back), so
it runs on an aligned copy and the view reaches ClassifHeadFunction.backward directly (test_gpu_guard_bands.b_classif)."""
import pytest
import torch

import test_gpu_guard_bands as T

HEAD_ENTRIES = ('mode_head_fwd', 'mode_head_bwd', 'mode_head_bwd_conf')
LOSS_ENTRIES = ('mode_head_fwd', 'mode_smooth_l1_masked', 'mode_head_bwd_loss')
CLASSIF_ENTRIES = ('mode_classif_train_fwd', 'mode_classif_train_bwd_amax')
CLASSIF_TWIN = 'mode_classif_train_bwd'  # what PlainTwins turns the second run's _amax call into

# (B, D4, H4, W4) -> what mode_head_loss_supported says of the shape at 4 x: the form the backward's routing takes
HEAD_ROWS = [(1, 8, 3, 8), (1, 16, 3, 8), (1, 64, 2, 8), (2, 64, 3, 16)]
HEAD_PIXELS = [(1, 8, 3, 7), (1, 16, 2, 7), (1, 48, 2, 7), (1, 64, 2, 7)]
HEAD_BORDER = [(1, 8, 3, 8), (1, 16, 3, 8), (1, 64, 2, 8), (1, 64, 2, 7)]
HEAD_LOSS = [(1, 8, 4, 8), (1, 16, 4, 8), (1, 64, 3, 8)]
ROUTING = dict([(s, 1) for s in HEAD_ROWS + HEAD_LOSS] + [(s, 0) for s in HEAD_PIXELS])

CLASSIF = [
    (1, 32, (3, 5, 40)),   # TC = 64, tile ragged in W (40 of 64) and in H (5 over the 4-row and the 8-row tiles)
    (2, 17, (2, 7, 64)),   # TC = 64 at full width, 17 channels, two samples
    (1, 32, (1, 9, 64)),   # TC = 64, D = 1: both depth halos outside
    (1, 32, (2, 10, 44)),  # TC = 64, ragged
    (1, 5, (1, 3, 72)),    # TC = 128 ragged, 5 channels, D = 1
    (1, 32, (2, 6, 132)),  # TC = 128, a second tile of 4 columns
    (1, 24, (3, 9, 76)),   # TC = 128 ragged, 24 channels
    (1, 31, (2, 9, 20)),   # TC = 32 ragged, 31 channels
    (2, 32, (4, 16, 8)),   # TC = 32: the volume of the 64 x 32 / 16-disparity model
    (1, 8, (2, 3, 4)),     # W = 4: one 16-byte piece per row
]
OFF_GRID = (1, 32, (3, 5, 40))


def b_head_rows(B, D4, H4, W4):
  return T.b_head(B, D4, H4, W4, 4, conf_grad=True, loss_supported=True)


def b_head_pixels(B, D4, H4, W4):
  return T.b_head(B, D4, H4, W4, 4, conf_grad=True, loss_supported=False)


def b_head_border(B, D4, H4, W4):
  return T.b_head(B, D4, H4, W4, 4, conf_grad=True, border=True, loss_supported=bool(ROUTING[(B, D4, H4, W4)]))


def b_classif_16b(B, C, vol, with_add):
  return T.b_classif(B, C, vol, with_add, clear_of_the_threshold=True)


def b_classif_off_grid(B, C, vol, with_add):
  return T.b_classif(B, C, vol, with_add, off_grid=True, clear_of_the_threshold=True)


_FIRST = len(T.CASES)
for _s in HEAD_ROWS:
  T.case('head_rows', HEAD_ENTRIES, b_head_rows, _s)
for _s in HEAD_PIXELS:
  T.case('head_pixels', HEAD_ENTRIES, b_head_pixels, _s)
for _s in HEAD_BORDER:
  T.case('head_border_%s' % ('rows' if ROUTING[_s] else 'pixels'), HEAD_ENTRIES, b_head_border, _s)
for _s in HEAD_LOSS:
  T.case('head_loss_rows', LOSS_ENTRIES, T.b_head_loss, _s)  # (b_head_loss asserts HF.head_loss_supported itself)
for _arith in ('f32', 'bf16x6'):
  for _i, _s in enumerate(CLASSIF):
    T.case('classif_16b', CLASSIF_ENTRIES, b_classif_16b, _s + (_i % 2 == 0,), _arith)
  T.case('classif_off_grid', CLASSIF_ENTRIES, b_classif_off_grid, OFF_GRID + (True,), _arith)
CASES = T.CASES[_FIRST:]
ALLOWED = {'head_loss_rows': set(LOSS_ENTRIES), 'classif_16b': set(CLASSIF_ENTRIES) | {CLASSIF_TWIN},
           'classif_off_grid': set(CLASSIF_ENTRIES) | {CLASSIF_TWIN}}


def test_the_cases_declare_their_entries():
  """CPU tier.  Together with the rest of the table they cover the launching ABI (the ledger of tests/test_guard_bands_host.py)."""
  assert len(CASES) == len(HEAD_ROWS) + len(HEAD_PIXELS) + len(HEAD_BORDER) + len(HEAD_LOSS) + 2 * (len(CLASSIF) + 1)
  assert set().union(*[c.entries for c in CASES]) == set(HEAD_ENTRIES) | set(LOSS_ENTRIES) | set(CLASSIF_ENTRIES)
  assert all(c in T.CASES for c in CASES) and len({c.id for c in T.CASES}) == len(T.CASES)
  for c in CASES:
    want = LOSS_ENTRIES if c.name == 'head_loss_rows' else (CLASSIF_ENTRIES if c.name.startswith('classif') else HEAD_ENTRIES)
    assert c.entries == frozenset(want), c.id
  import test_guard_bands_host as G
  assert set().union(*[c.entries for c in CASES]) <= G.launching_entries()


def test_the_routing_table_is_what_the_library_says():
  """CPU tier (mode_head_loss_supported is host code): every head shape takes the form of the backward it is listed under, and the
  classifier widths cover the three tile widths of the 16-byte kernels, each with a ragged tile."""
  import mode_hip
  lib = mode_hip.lib()
  for (B, D4, H4, W4), want in ROUTING.items():
    assert lib.mode_head_loss_supported(B, D4, H4, W4, 4 * D4, 4 * H4, 4 * W4) == want, (B, D4, H4, W4)
  assert set(HEAD_BORDER) <= set(ROUTING) and {s[1] for s in ROUTING} == {8, 16, 48, 64}
  tile_cols = lambda W: 128 if W > 64 else (64 if W > 32 else 32)  # csrc/classif_head.hip
  assert all(vol[2] % 4 == 0 for _, _, vol in CLASSIF + [OFF_GRID])
  assert {tile_cols(vol[2]) for _, _, vol in CLASSIF} == {32, 64, 128}
  assert {tile_cols(vol[2]) for _, _, vol in CLASSIF if vol[2] % tile_cols(vol[2])} == {32, 64, 128}


@pytest.fixture
def stop_at_a_gpu_fault():
  """As test_gpu_guard_bands._stop_at_a_gpu_fault (not autouse here: this file has CPU-tier tests): if the device no longer answers
  after a test, the session ends there."""
  yield
  try:
    torch.cuda.synchronize()
  except RuntimeError as e:
    pytest.exit('the GPU reported an error after this test; nothing more is started on it: %s' % e, returncode=3)


@pytest.mark.gpu
@pytest.mark.parametrize('c', CASES, ids=[c.id for c in CASES])
def test_guarded_heads(c, monkeypatch, stop_at_a_gpu_fault):
  rec, stats = T.run_case(c, monkeypatch)
  assert c.entries, 'every case declares the entries it is there to launch'
  missing = sorted(c.entries - set(rec.launched))
  assert not missing, 'declared but not launched: %s (launched: %s)' % (missing, sorted(rec.launched))
  assert set(rec.launched) <= ALLOWED.get(c.name, set(HEAD_ENTRIES)), sorted(rec.launched)
  T.STATS['allocations'] += sum(stats['allocations'])
  T.STATS['launches'] += sum(rec.launched.values())
  T.STATS['cases'] += 1
  print('  %d guarded allocations, %d launching calls' % (sum(stats['allocations']), sum(rec.launched.values())))
  print('LAUNCHED %s %s' % (c.id, ' '.join(sorted(rec.launched))))
