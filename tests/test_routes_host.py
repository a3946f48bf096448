"""Host tier (no GPU): the route functions of mode_hip.functional -- the one place per layer family where the kernel is chosen.

_conv3d_route and _conv2d_route ask the library's host-only predicates (mode_conv3d_split_shape_supported,
mode_conv2d_split_shape_supported) and the module's switches; every call site of the family asks them.  The table below states the
routes of the shapes the GPU trace test (tests/test_gpu_routes.py) runs, and of one volume beyond the split kernels' 32-bit contract
(the probe of tests/test_size_contracts_host.py: 8 -> 8 at 1024 x 128 x 512, where 32 DHW reaches 2^31)."""
import pytest

from mode_hip import functional as HF

FWD, BWD_DATA, BWD_WEIGHT = 0, 1, 2
S1 = (32, 32, 1, (6, 10, 40))


@pytest.fixture(autouse=True)
def _switches():
  prev = HF.CONV_ARITH
  yield
  HF.set_conv_arith(prev)


# (ci, co, stride, vol, which, arithmetic, f16 argument) -> route
ROUTES_3D = [(S1 + (which, 'bf16x6', True), 'split_f16') for which in (FWD, BWD_DATA, BWD_WEIGHT)] + \
            [(S1 + (which, 'bf16x6', False), 'split') for which in (FWD, BWD_DATA, BWD_WEIGHT)] + \
            [(S1 + (which, 'f32', True), 'f32') for which in (FWD, BWD_DATA, BWD_WEIGHT)] + [
    ((8, 8, 1, (1023, 128, 512), BWD_DATA, 'bf16x6', True), 'split_f16'),   # the last volume inside the contract of the input gradient
    ((8, 8, 1, (1024, 128, 512), BWD_DATA, 'bf16x6', True), 'f32'),         # ... and the first beyond it: the fp32 kernel, not a failure
    ((32, 64, 2, (4, 8, 64), FWD, 'bf16x6', True), 's2_split'),             # stride 2 has no fp16 form: f16 is not looked at
    ((32, 64, 2, (4, 8, 64), BWD_DATA, 'bf16x6', False), 's2_split'),
    ((32, 64, 2, (4, 8, 64), BWD_WEIGHT, 'bf16x6', True), 's2_split'),
    ((32, 64, 2, (4, 8, 64), FWD, 'f32', True), 'f32'),
    ((20, 40, 1, (5, 7, 33), FWD, 'bf16x6', True), 'f32'),                  # 20 input channels: off the forward's grid
    ((20, 1, 1, (3, 5, 33), FWD, 'bf16x6', True), 'f32'),                   # the single-channel head
    ((20, 1, 1, (3, 5, 33), BWD_DATA, 'bf16x6', True), 'f32'),
    ((20, 1, 1, (3, 5, 33), BWD_WEIGHT, 'bf16x6', True), 'f32'),
]


@pytest.mark.parametrize('case,want', ROUTES_3D, ids=[str(c) for c, _ in ROUTES_3D])
def test_conv3d_route(case, want):
  ci, co, stride, vol, which, arith, f16 = case
  HF.set_conv_arith(arith)
  assert HF._conv3d_route(ci, co, stride, which, vol, f16) == want


def test_the_3d_callers_pass_their_own_switch(monkeypatch):
  """conv3d_s1_f16 is the training question (CONV3D_S1_F16); the transposed convolution asks as the stride-2 input gradient of the
  convolution cout -> cin over the doubled volume."""
  HF.set_conv_arith('bf16x6')
  monkeypatch.setattr(HF, 'CONV3D_S1_F16', True)
  assert HF.conv3d_s1_f16(32, 32, FWD, (6, 10, 40)) is True and HF.conv3d_s1_f16(32, 32, FWD) is True
  assert HF.conv3d_s1_f16(20, 40, FWD, (5, 7, 33)) is False
  monkeypatch.setattr(HF, 'CONV3D_S1_F16', False)
  assert HF.conv3d_s1_f16(32, 32, FWD, (6, 10, 40)) is False
  seen = []
  real = HF._conv3d_route
  monkeypatch.setattr(HF, '_conv3d_route', lambda *a: (seen.append(a), real(*a))[1])
  assert HF._deconv_split3d(64, 32, (6, 16, 32)) is True
  assert seen == [(32, 64, 2, BWD_DATA, (12, 32, 64), False)]
  HF.set_conv_arith('f32')
  assert HF._deconv_split3d(64, 32, (6, 16, 32)) is False


# (ci, co, H, W, dilation, which, arithmetic, f16 argument) -> route
ON_GRID = [((32, 32, 16, 32, dil, which, 'bf16x6', f16), 'split_f16' if f16 else 'split')
           for dil in (1, 2) for which in (FWD, BWD_DATA, BWD_WEIGHT) for f16 in (True, False)]
OFF_GRID = [((24, 40, 9, 33, 1, FWD, 'bf16x6', True), 'f32'),        # 24 -> 40 is off the 16-channel grid of the forward ...
            ((24, 40, 9, 33, 1, BWD_DATA, 'bf16x6', True), 'f32'),   # ... and of the input gradient;
            ((24, 40, 9, 33, 1, BWD_WEIGHT, 'bf16x6', False), 'split'),      # the weight gradient masks its blocks: any channel counts
            ((24, 40, 9, 33, 1, BWD_WEIGHT, 'bf16x6', True), 'split_f16')]
F32 = [((32, 32, 16, 32, dil, which, 'f32', True), 'f32') for dil in (1, 2) for which in (FWD, BWD_DATA, BWD_WEIGHT)]
ROUTES_2D = ON_GRID + OFF_GRID + F32


@pytest.mark.parametrize('case,want', ROUTES_2D, ids=[str(c) for c, _ in ROUTES_2D])
def test_conv2d_route(case, want):
  ci, co, H, W, dil, which, arith, f16 = case
  HF.set_conv_arith(arith)
  assert HF._conv2d_route(ci, co, H, W, dil, which, f16) == want


def test_the_training_sites_of_the_3x3_family_ask_conv2d_f16(monkeypatch):
  """_conv2d_f16 is what the training sites pass as f16: CONV2D_F16 and the bf16x6 arithmetic and the caller's own flag."""
  HF.set_conv_arith('bf16x6')
  monkeypatch.setattr(HF, 'CONV2D_F16', True)
  assert HF._conv2d_f16(True) is True and HF._conv2d_f16(False) is False
  monkeypatch.setattr(HF, 'CONV2D_F16', False)
  assert HF._conv2d_f16(True) is False
  monkeypatch.setattr(HF, 'CONV2D_F16', True)
  HF.set_conv_arith('f32')
  assert HF._conv2d_f16(True) is False


def test_call_resolves_check_and_lib_at_call_time(monkeypatch):
  """_call('mode_x', ...) is check(lib().mode_x(...), 'mode_x') through the module's globals: a test that replaces either sees every entry."""
  seen = []

  class Lib(object):
    def mode_probe(self, a, b):
      seen.append(('entry', a, b))
      return 7

  monkeypatch.setattr(HF, 'lib', lambda: Lib())
  monkeypatch.setattr(HF, 'check', lambda rc, what: seen.append(('check', rc, what)))
  HF._call('mode_probe', 1, 2)
  assert seen == [('entry', 1, 2), ('check', 7, 'mode_probe')]
