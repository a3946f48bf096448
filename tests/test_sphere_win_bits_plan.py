"""Host: the table of tests/test_gpu_sphere_win_bits.py reaches every class of windowed kernel, so that no case of it passes vacuously.

The planners run on the host (csrc/sphere_plan.hip), so this needs no GPU: the forward / weight-gradient plan of the table has compact,
mid and wrap tiles and polar items, its adjoint plan has good tiles of the six-source class, and every input-gradient case has
channel counts the windowed kernel takes.  The small table of the two extra input-gradient cases is good adjoint tiles but for the one
whose lists weigh more than the fp16 form can take."""
import make_golden_sphere_win_bits as G
from mode_hip import functional as HF
from oracle import mode_ref


def test_the_table_has_every_tile_class():
  pos = mode_ref.sphere_position(*G.TABLE, 'Cassini').contiguous()
  plan = HF.sphere_plan(pos, 3, 3)
  assert plan is not None and HF._plan_usable(plan)
  n_small, n_mid, n_wrap = plan.counts
  assert n_small > 0 and n_mid > 0 and n_wrap > 0, plan.counts
  assert plan.polar is not None and plan.polar.n > 0  # polar items
  aplan = HF.sphere_adjplan(pos, 3, 3)
  assert aplan is not None and aplan.ngood > 0
  six = (aplan.tiles.view(-1, 4)[:, 3] >> 16) & 1
  assert 0 < int(six.sum()) < aplan.ngood  # both the four- and the six-source class
  assert aplan.nbad > 0  # and tiles left to the gather kernel's list form


def test_the_small_table_is_windowed_input_gradient_but_for_its_heavy_tile():
  pos = mode_ref.sphere_position(*G.SMALL_TABLE, 'Cassini').contiguous()
  assert tuple(pos.shape[2:]) == (64, 32)
  full = HF.sphere_adjplan(pos, 3, 3, f16=False)  # three bf16 pieces: every tile good, nothing for the gather kernel
  assert full is not None and full.ngood == 8 and full.bad_ids is None and full.nbad == 0
  aplan = HF.sphere_adjplan(pos, 3, 3, f16=True)
  # two fp16 pieces: seven of the eight tiles good; tile (0, 0), whose adjoint lists weigh up to 2.18 (beyond the fp16 headroom of 2 - 2^-10,
  # tests/test_sphere_f16_ref_host.py), is the four 64-pixel runs of the stored rows 0 .. 3 for the gather kernel
  assert aplan is not None and aplan.ngood == 7 and aplan.nbad == 4 and aplan.bad_ids.tolist() == [0, 1, 2, 3]
  six = (aplan.tiles.view(-1, 4)[:, 3] >> 16) & 1
  assert 0 < int(six.sum()) < aplan.ngood
  assert not HF._plan_usable(HF.sphere_plan(pos, 3, 3))  # no compact tile: the model keeps it off the other two windowed passes


def test_every_case_reaches_its_kernel():
  for case in G.FWD + G.EVAL + G.BWD_WEIGHT:
    assert tuple(case[:2]) == G.TABLE
  for case in G.FWD + G.EVAL + G.BWD_DATA + G.BWD_WEIGHT:
    assert case[2] <= 2 and max(case[3], case[4]) <= 64
  for case in G.BWD_DATA:
    assert tuple(case[:2]) in (G.TABLE, G.SMALL_TABLE)
    assert HF.lib().mode_sphere_conv_bwd_data_win_supported(case[3], case[4], case[5]) == 1
  assert {tuple(case[:2]) for case in G.BWD_DATA} == {G.TABLE, G.SMALL_TABLE}
