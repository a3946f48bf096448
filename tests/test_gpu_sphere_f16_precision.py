"""GPU (-m gpu): the fp16 spherical training entries -- mode_sphere_conv_fwd_win_split_f16, mode_sphere_conv_bwd_data_win_split_f16,
mode_sphere_conv_bwd_weight_win_split_f16: what a default training step runs the spherical layers on -- against the componentwise
contract of csrc/split_arith.h, judged per element as tests/test_gpu_split_precision.py judges the other MFMA kernels.

Cases, references, the arithmetic map of every role and the thresholds are those of tests/split_ref.py (SPHERE_F16_CASES, sphere_f16_roles);
tests/test_sphere_f16_ref_host.py shows on the CPU that a faithful kernel with an fp32 accumulator stays below T / 1.5 on every one of
them and that a mutant confined to one region, or one structural fault, exceeds T.  Switches: CONV_ARITH 'bf16x6', SPHERE_FWD_F16 =
SPHERE_BWD_F16 = True, SPHERE_FWD_MIN_WG = SPHERE_BWD_SPLIT_MIN_WG = 0 (the small tables too), restored afterwards.

Per role: the entries that launched, by name (the recorder of tests/test_gpu_size_contracts.py; the gather kernel's list form exactly when
the adjoint plan has bad tiles); a finite output, exactly zero where every product is zero; per PART (an arithmetic and the pixels it
covers) the rms over the part and the worst slice -- along every axis, and every window class / slot class as a slice of its own -- both
<= T; a second call gives the same bits; forward and input gradient run once more with the maximum read from a tag a producer left
(known_abs_max) instead of an abs_max pass: the same bits.  The weight gradient runs three times -- gy zeroed on the polar pixels, gy
zeroed on the compact pixels, unmasked -- and the two masked results add up to the unmasked one within the three runs' own thresholds.
No expected failures: a kernel that misses T here, where the host tier says a faithful one meets T / 1.5, is a finding.

MEASURED on an MI355X (one run of this file; T is computed, rms and worst slice are measured; per role, part and kind of data the case
with the least room, i.e. the largest worst slice / T):

role                             part         data                          T    rms  worst  at the shape (of n), slice
forward                          fp16 pieces  unit variance             32.326  0.077  0.092  16x32x1x16x32x1 (3), 3 @ 9
forward                          fp16 pieces  six decades along a row    0.791  0.126  0.210  33x66x1x32x64x2 (3), 1 @ 31
input gradient                   fp16 tiles   unit variance             23.552  0.071  0.086  32x64x1x32x32x1 (1), 2 @ 0
input gradient                   fp16 tiles   six decades along a row    0.542  0.105  0.169  32x64x1x32x32x1 (1), 1 @ 2
input gradient                   fp16 tiles   gradient-sized            23.552  0.071  0.088  32x64x1x32x32x1 (1), 2 @ 0
input gradient                   fp16 tiles   plateau                   26.775  0.100  0.168  32x64x1x16x16x1 (1), 1 @ 5
input gradient                   fp32 tiles   unit variance              1.537  0.447  0.655  32x64x1x32x32x1 (1), 3 @ 0
input gradient                   fp32 tiles   six decades along a row    2.272  0.588  0.885  32x64x1x32x32x1 (1), 1 @ 15
input gradient                   fp32 tiles   gradient-sized             1.520  0.443  0.646  32x64x1x32x32x1 (1), 3 @ 0
input gradient                   fp32 tiles   plateau                    2.224  0.830  1.646  32x64x1x16x16x1 (1), 1 @ 3
weight gradient, compact pixels  fp16 pieces  unit variance              5.828  0.014  0.016  64x128x1x16x32x1 (2), 3 @ 1
weight gradient, compact pixels  fp16 pieces  gradient-sized             5.713  0.014  0.015  64x128x1x16x32x1 (2), 3 @ 1
weight gradient, polar pixels    bf16 pieces  unit variance              0.336  0.061  0.071  64x128x1x16x32x1 (2), 3 @ 1
weight gradient, polar pixels    bf16 pieces  gradient-sized             0.337  0.060  0.069  64x128x1x16x32x1 (2), 3 @ 1
weight gradient                  both         unit variance              1.387  0.017  0.019  33x66x1x32x64x2 (2), 3 @ 1
weight gradient                  both         gradient-sized             1.406  0.017  0.019  33x66x1x32x64x2 (2), 3 @ 1
weight gradient                  fp16 pieces  unit variance             17.289  0.038  0.044  16x32x1x16x32x1 (1), 3 @ 1
weight gradient                  fp16 pieces  six decades along a row  109.825  0.616  0.663  16x32x1x16x32x1 (1), 1 @ 7
weight gradient                  fp16 pieces  gradient-sized            17.126  0.039  0.044  16x32x1x16x32x1 (1), 3 @ 1

(family sphere, fp16 entries.  The fp32 tiles of the input gradient are the one bad tile of the 32 x 64 table, 256 pixels per channel, on the
gather kernel's list form, in units of 2^-24 under the three-piece T; on the plateau every pixel of a channel holds the same sum, so the
accumulator's rounding does not average over a slice: 1.646 of 2.224.  The masked weight-gradient runs add up to the unmasked one
within 0.009 - 0.010 units of 2^-22, against 9.4 - 56 allowed.)
"""
import pytest
import torch

import cpu_threads
import mode_hip
import split_ref as S
from mode_hip import functional as HF
from test_gpu_size_contracts import recorder  # noqa: F401  (the fixture that records the launching entries by name)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SWITCHES = ('SPHERE_FWD_F16', 'SPHERE_BWD_F16', 'SPHERE_FWD_MIN_WG', 'SPHERE_BWD_SPLIT_MIN_WG')
COMPUTE = ('mode_sphere_conv',)
FWD, BWD, BWW = ('mode_sphere_conv_fwd_win_split_f16', 'mode_sphere_conv_bwd_data_win_split_f16', 'mode_sphere_conv_bwd_weight_win_split_f16')
LIST = 'mode_sphere_conv_bwd_data_adj_list'

# The judged roles of every shape, written out: a planner or a route that starts to say no must fail the test, not empty it.
WG3 = ('weight gradient, compact pixels', 'weight gradient, polar pixels', 'weight gradient')
JUDGED = {
    (16, 32, 1, 16, 32, 1): ('forward', 'weight gradient'),  # (four compact tiles and no other: one run of the weight gradient)
    (33, 66, 1, 32, 64, 2): ('forward',) + WG3,
    (64, 128, 1, 16, 32, 1): ('forward',) + WG3,
    (32, 64, 1, 32, 32, 1): ('input gradient',),
    (32, 64, 1, 16, 16, 1): ('input gradient',),
}
# ... and the parts of the input gradient: the 32 x 64 table has seven good tiles (fp16 pieces) and one bad one (fp32 gather)
PARTS = {'input gradient': ['fp16 tiles', 'fp32 tiles']}


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
  assert torch.cuda.is_available(), 'GPU tests need a GPU'
  mode_hip.lib()
  torch.set_num_threads(cpu_threads.usable_cores())


@pytest.fixture
def switches():
  keep = (HF.CONV_ARITH,) + tuple(getattr(HF, n) for n in SWITCHES)
  HF.set_conv_arith('bf16x6')
  HF.SPHERE_FWD_F16 = HF.SPHERE_BWD_F16 = True
  HF.SPHERE_FWD_MIN_WG = HF.SPHERE_BWD_SPLIT_MIN_WG = 0
  yield
  HF.set_conv_arith(keep[0])
  for n, v in zip(SWITCHES, keep[1:]):
    setattr(HF, n, v)


_REFS = {}


def _reference(case):
  """The float64 references of a case, computed once for the module and left unchanged."""
  if case not in _REFS:
    _REFS[case] = S.sphere_f16_roles(case)
  return _REFS[case]


def _launch(case, role, t):
  """(the entries that must run, run(tagged) -> the result on the device).  tagged: the maximum of the activation / gradient comes from a
  tag left beside the tensor (HF._tag_amax, as BatchNorm's kernels leave it) instead of the abs_max pass of the first call."""
  ih, iw, B, ci, co, g = case.shape
  d = lambda v: v.to(DEV)
  pos = d(t['pos'])
  H, W = pos.shape[2:]
  w = d(t['w'])

  def fresh(src, tagged):
    v = src.clone()
    if tagged:
      HF._tag_amax(v, HF.abs_max(src))
      assert HF.known_abs_max(v) is not None
    else:
      assert HF.known_abs_max(v) is None
    return v

  if role.name == 'forward':
    x = d(t['x'])
    return [FWD], lambda tagged=False: HF.sphere_conv_fwd(fresh(x, tagged), pos, w, torch.full((B, co, H, W), float('nan'), device=DEV), (1, 1), g, f16=True)
  if role.name == 'input gradient':
    aplan = HF.sphere_adjplan(pos, 3, 3, f16=True)
    assert aplan is not None and HF.lib().mode_sphere_conv_bwd_data_win_supported(ci, co, g) == 1
    gyt = HF.transpose_planes(d(role.gy))

    def run(tagged=False):
      gxt = torch.full((B, ci, W, H), float('nan'), device=DEV)
      HF.sphere_conv_bwd_data_t(fresh(gyt, tagged), pos, w, gxt, g)
      return HF.transpose_planes(gxt)
    return [BWD] + ([LIST] if aplan.nbad else []), run
  gy, x = d(role.gy), d(t['x'])
  return [BWW], lambda tagged=False: HF.sphere_conv_bwd_weight(gy.clone(), pos, x.clone(), torch.zeros((co, ci // g, 3, 3), device=DEV), (1, 1), g)


@pytest.mark.parametrize('case', S.SPHERE_F16_CASES, ids=S.case_id)
def test_fp16_spherical_entry_keeps_the_componentwise_contract(case, switches, recorder):
  roles, tensors = _reference(case)
  shape = 'x'.join(str(v) for v in case.shape)
  maps = tensors['maps']
  assert not bool(maps.fwd_fp32.any())
  judged, missed, got_of = [], [], {}
  for role in roles:
    entries, run = _launch(case, role, tensors)
    del recorder.names[:]
    got = run()
    torch.cuda.synchronize()
    ran = [n for n in recorder.names if n.startswith(COMPUTE)]
    assert ran == entries, (S.case_id(case), role.name, ran)
    if role.name == 'input gradient':
      assert (LIST in entries) == bool((~maps.good).any())
      assert [p.name for p in role.parts] == PARTS['input gradient']
    assert bool(torch.isfinite(got).all()), (S.case_id(case), role.name, 'not finite: %d elements' % int((~torch.isfinite(got)).sum()))
    assert torch.equal(run(), got), (S.case_id(case), role.name, 'a second call gives other bits')
    if not role.name.startswith('weight gradient'):
      assert torch.equal(run(tagged=True), got), (S.case_id(case), role.name, 'the maximum from a tag gives other bits than the one from a pass')
    got_of[role.name] = got.cpu().double()
    for part in role.parts:
      whole, worst = S.part_measure(role, part, got)
      print('SPHEREF16 | %s | %s | %s | %s | %s | T %.3f | rms %.3f | worst slice %.3f (%s @ %s)' %
            (shape, role.name, part.name, case.kind, ' + '.join(e[5:] for e in entries), part.T, whole, worst.rms, worst.axis, worst.index))
      if not (whole <= part.T and worst.rms <= part.T):
        missed.append((role.name, part.name, 'T %.3f' % part.T, 'rms %.3f' % whole, worst))
    judged.append(role.name)
  want = [n for n in ('forward', 'input gradient') + WG3 if n in JUDGED[case.shape]]
  skip = {'forward'} if case.kind == 'gradient-sized' else set()  # (tests/split_ref.py: no forward reads a gradient, ...
  if case.kind == 'six decades along a row' and maps.cls.numel() > S.SPHERE_WGRAD_DECADES_MAX_PIXELS:
    skip |= set(WG3)  # ... and the six-decades weight gradient up to 512 pixels)
  assert judged == [n for n in want if n not in skip] and judged, (S.case_id(case), judged)
  if all(n in got_of for n in WG3):
    # the two masked runs add up to the unmasked one: each is within its own threshold of its float64 value, those values add up
    # exactly, den of a masked run is <= den of the unmasked one and a unit of 2^-24 is a quarter of one of 2^-22 (Minkowski on the rms)
    r1, r2, r3 = (next(r for r in roles if r.name == n) for n in WG3)
    u = S.units(got_of[WG3[0]] + got_of[WG3[1]], got_of[WG3[2]], r3.den, 'f16x3')
    bound = r1.parts[0].T + r2.parts[0].T / 4 + r3.parts[0].T
    print('SPHEREF16 | %s | masked runs against the unmasked one | %s | rms %.3f of %.3f allowed' % (shape, case.kind, S.rms(u), bound))
    assert S.rms(u) <= bound, (S.case_id(case), S.rms(u), bound)
  assert not missed, (S.case_id(case), missed)
