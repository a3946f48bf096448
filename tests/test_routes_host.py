"""Host tier (no GPU): the route functions of mode_hip.functional -- the one place per layer family where the kernel is chosen.

_conv3d_route and _conv2d_route ask the library's host-only predicates (mode_conv3d_split_shape_supported,
mode_conv2d_split_shape_supported) and the module's switches; every call site of the family asks them.  The table below states the
routes of the shapes the GPU trace test (tests/test_gpu_routes.py) runs, and of one volume beyond the split kernels' 32-bit contract
(the probe of tests/test_size_contracts_host.py: 8 -> 8 at 1024 x 128 x 512, where 32 DHW reaches 2^31).

The spherical routes (_sphere_fwd_route, _sphere_bwd_data_route, _sphere_bwd_data_t_route, _sphere_bwd_weight_route) ask the tile
planners, which run on the host, so their table below runs on CPU tables: every kind of table crossed with every switch the routes read.
Its values were written from the ladders the operators held inline before the routes existed; tests/test_gpu_routes.py is the proof on
the GPU that they are those."""
import pytest
import torch

import sphere_tables as T
from mode_hip import functional as HF
from models.basic.spherical_conv.sphere_conv import make_sphere_position

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


# ------------------------------------------------------------------------------------------------ the spherical family
SPHERE_TABLES = {
    'cassini': lambda: make_sphere_position(96, 192, 'Cassini', (3, 3)),  # 192 x 96: a plan usable as a whole, 63 good adjoint tiles
    'erp': lambda: make_sphere_position(96, 192, 'ERP', (3, 3)),          # 96 x 192: no plan of its own, its transpose is the one above
    'perturbed': T.perturbed,               # 192 x 96, tall-window tiles without polar items: the pixel list; neither kind of table
    'affine 0.5': lambda: T.affine(0.5),    # 192 x 16 (4 tile columns), no compact tile -- but its TRANSPOSE has a usable plan: ERP-like
    'small': lambda: make_sphere_position(32, 64, 'Cassini', (3, 3)),     # 64 x 32: no compact tile and no usable transpose: forward only
}
WG0 = {'SPHERE_FWD_MIN_WG': 0, 'SPHERE_BWD_SPLIT_MIN_WG': 0}
SPHERE_SWITCHES = {
    'wg0': WG0, 'wg200': {'SPHERE_FWD_MIN_WG': 200, 'SPHERE_BWD_SPLIT_MIN_WG': 200}, 'nchw': dict(WG0, SPHERE_LAYOUT='nchw'),
    'nopolar': dict(WG0, SPHERE_POLAR=False), 'scatter': dict(WG0, SPHERE_BWD_DATA='scatter'), 'no bwd_data_t': dict(WG0, SPHERE_BWD_DATA_T=False),
    'bww gather': dict(WG0, SPHERE_BWD_WEIGHT='gather'), 'f32': dict(WG0, CONV_ARITH='f32'), 'no split': dict(WG0, SPHERE_BWD_DATA_SPLIT=False),
}
# table -> switches -> (forward, NCHW input gradient as sphere_conv_backward_cuda asks for it [/ the plane-transposed route behind it],
# weight gradient, plane-transposed input gradient asked directly) at B = 1, 32 -> 32, stride 1; switch sets not listed: as 'wg0'
W, A = 'window', 'adjoint'
SPHERE_ROUTES = {
    'cassini': {
        'wg0': ('window', 'copies_t/window', 'window', W),
        'wg200': ('gather', 'copies_t/adjoint', 'window', A),        # 72 forward workgroups, 63 good adjoint tiles; the weight gradient has no floor
        'nchw': ('window', 'adjoint', 'window', W),                  # no copies are made: nothing to hand the input gradient
        'nopolar': ('window', 'adjoint', 'window', W),               # the plan is not usable as a whole: not 'copies'; both passes run it all the same
        'scatter': ('window', 'scatter', 'window', W),
        'no bwd_data_t': ('window', 'adjoint', 'window', W),
        'bww gather': ('window', 'copies_t/window', 'gather', W),
        'f32': ('window', 'copies_t/adjoint', 'window', A),
        'no split': ('window', 'copies_t/adjoint', 'window', A),
    },
    'erp': {                                                          # (the table itself has no adjoint plan: 96 rows)
        'wg0': ('native_t', 'native_t/window', 'native_t', A),
        'wg200': ('gather', 'native_t/adjoint', 'native_t', A),      # a small batch: gather forward, `_t` gradients
        'nchw': ('gather', 'adjoint', 'gather', A),
        'nopolar': ('gather', 'adjoint', 'gather', A),               # the transpose's plan is not usable as a whole either
        'scatter': ('gather', 'scatter', 'native_t', A),             # the forward asks sphere_t_supported, the weight gradient sphere_native_t alone
        'no bwd_data_t': ('native_t', 'adjoint', 'native_t', A),
        'bww gather': ('gather', 'native_t/window', 'gather', A),
        'f32': ('native_t', 'native_t/adjoint', 'native_t', A),
        'no split': ('native_t', 'native_t/adjoint', 'native_t', A),
    },
    'perturbed': {
        'wg0': ('window', 'adjoint', 'window', W),
        'wg200': ('gather', 'adjoint', 'window', A),
        'scatter': ('window', 'scatter', 'window', W),
        'bww gather': ('window', 'adjoint', 'gather', W),
        'f32': ('window', 'adjoint', 'window', A),
        'no split': ('window', 'adjoint', 'window', A),
    },
    'affine 0.5': {                                                   # (16 rows in the transpose: no adjoint plan behind native_t; 4 good tiles of its own)
        'wg0': ('native_t', 'native_t/adjoint', 'native_t', W),
        'wg200': ('gather', 'native_t/adjoint', 'native_t', A),
        'nchw': ('window', 'adjoint', 'gather', W),                  # its own plan: the forward runs it, the weight gradient drops it (no compact tile)
        'scatter': ('window', 'scatter', 'native_t', W),
        'no bwd_data_t': ('native_t', 'adjoint', 'native_t', W),
        'bww gather': ('window', 'native_t/adjoint', 'gather', W),
        'f32': ('native_t', 'native_t/adjoint', 'native_t', A),
        'no split': ('native_t', 'native_t/adjoint', 'native_t', A),
    },
    'small': {
        'wg0': ('window', 'adjoint', 'gather', W),
        'wg200': ('gather', 'adjoint', 'gather', A),
        'scatter': ('window', 'scatter', 'gather', W),
        'f32': ('window', 'adjoint', 'gather', A),
        'no split': ('window', 'adjoint', 'gather', A),
    },
}
_tables = {}


def _sphere_table(name):
  if name not in _tables:
    _tables[name] = SPHERE_TABLES[name]().contiguous()
  return _tables[name]


def _sphere_routes(pos, B, ci, co, groups, stride):
  """The four answers for one layer, each checked for the plan or table it came with."""
  st, same = (stride, stride), stride == 1
  plan, post = HF.sphere_plan(pos, 3, 3), HF._transposed_table(pos)
  weight = torch.empty(co, ci // groups, 3, 3)

  def behind(table):
    route, aplan = HF._sphere_bwd_data_t_route(table, 3, 3, B, ci, co, groups, *table.shape[2:])
    assert aplan is (HF.sphere_adjplan(table, 3, 3) if route == 'window' else None)
    return route
  fwd, got = HF._sphere_fwd_route(pos, weight, B, groups, st, same, honour_switch=True)
  assert got is {'window': plan, 'native_t': post, 'gather': None}[fwd]
  gyt = HF.sphere_grads_want_transposed_gy(pos, 3, 3, st, same)
  assert gyt == (same and HF.sphere_uses_transposed_copies(pos, 3, 3))
  bwd, got = HF._sphere_bwd_data_route(pos, 3, 3, st, same, True, gyt)
  assert got is (post if bwd == 'native_t' else None)
  if bwd in ('native_t', 'copies_t'):
    bwd += '/' + behind(post if bwd == 'native_t' else pos)
  bww, got = HF._sphere_bwd_weight_route(pos, 3, 3, st, same)
  assert got is {'window': plan, 'native_t': post, 'gather': None}[bww]
  return fwd, bwd, bww, behind(pos)


@pytest.mark.parametrize('switches', sorted(SPHERE_SWITCHES))
@pytest.mark.parametrize('table', sorted(SPHERE_TABLES))
def test_sphere_routes(monkeypatch, table, switches):
  for k, v in SPHERE_SWITCHES[switches].items():
    monkeypatch.setattr(HF, k, v)
  pos = _sphere_table(table)
  want = SPHERE_ROUTES[table].get(switches, SPHERE_ROUTES[table]['wg0'])
  assert _sphere_routes(pos, 1, 32, 32, 1, 1) == want
  # 32 -> 48 in two groups: 24 output channels per group are off the windowed input gradient's grid; nothing else asks the channels
  assert _sphere_routes(pos, 1, 32, 48, 2, 1) == (want[0], want[1].replace('/window', '/adjoint'), want[2], A)
  # stride 2: no windowed kernel and no `_t` operator in any pass (the directly asked plane-transposed route knows no stride)
  assert _sphere_routes(pos, 1, 32, 32, 1, 2) == ('gather', 'scatter' if switches == 'scatter' else 'adjoint', 'gather', want[3])


def test_the_three_table_questions_are_one_answer(monkeypatch):
  """_sphere_layout is asked once per table; sphere_native_t and sphere_uses_transposed_copies are its two halves, and both read
  SPHERE_LAYOUT and SPHERE_POLAR when they are called."""
  cas, erp, per = (_sphere_table(n) for n in ('cassini', 'erp', 'perturbed'))
  assert HF._sphere_layout(cas, 3, 3) == ('copies', HF.sphere_plan(cas, 3, 3))
  kind, post = HF._sphere_layout(erp, 3, 3)
  assert kind == 'native_t' and post is HF._transposed_table(erp) and HF.sphere_native_t(erp, 3, 3) is post
  assert HF._sphere_layout(per, 3, 3) == (None, HF.sphere_plan(per, 3, 3)) and HF.sphere_native_t(per, 3, 3) is None
  assert HF._sphere_layout(cas, 5, 5) == (None, None)
  monkeypatch.setattr(HF, 'SPHERE_POLAR', False)
  assert HF._sphere_layout(cas, 3, 3) == (None, HF.sphere_plan(cas, 3, 3)) and not HF.sphere_uses_transposed_copies(cas, 3, 3)
  monkeypatch.setattr(HF, 'SPHERE_POLAR', True)
  monkeypatch.setattr(HF, 'SPHERE_LAYOUT', 'nchw')
  assert HF._sphere_layout(erp, 3, 3) == (None, None) and HF.sphere_native_t(erp, 3, 3) is None


def test_sphere_win_geometry_is_the_rule_of_every_site():
  assert HF.sphere_win_geometry((1, 1), 3, 3, True) and HF.sphere_win_geometry([1, 1], 3, 3, True)
  assert not HF.sphere_win_geometry((2, 2), 3, 3, True) and not HF.sphere_win_geometry((1, 2), 3, 3, True)
  assert not HF.sphere_win_geometry((1, 1), 5, 5, True) and not HF.sphere_win_geometry((1, 1), 3, 3, False)
