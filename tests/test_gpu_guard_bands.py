"""GPU (-m gpu): no kernel reads or writes outside the buffers it was given -- the operator table of tests/guard_bands.py.

One case per family of launching C-ABI entries.  A case builds seeded standard-normal inputs, `place`s them between guard zones, runs
the operator through mode_hip.functional (whose own outputs, workspaces, weight packs and tables are then guarded too) under both guard
fills (guard_bands.under_two_fills: guards intact, outputs bit-equal between the fills, outputs finite) and compares the result with
the float64 reference and the bound of the operator's own test (named next to each case).  A recording stand-in for the library handle
verifies that the case launched the entries it declares; tests/test_guard_bands_host.py (CPU tier) verifies that the declarations cover
every launching entry of mode_hip.SIGNATURES.  Three whole paths (a tiny training step, its eval forward, a ModeFusion forward) run in
the same way: that is where a workspace undersized for the real call sequence shows.

Tensors that torch's own operators produce inside the host code are not intercepted (guard_bands' docstring).  Nothing here tries to
make a kernel fault: a wrong kernel damages a guard or changes a value, and the test says which buffer.
"""
import collections
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import guard_bands as GB

import mode_hip
from mode_hip import functional as HF

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


class RecordingLib(object):
  """Stands in for the ctypes handle (like test_gpu_repeat.PoisoningLib): counts the calls of every launching entry."""

  def __init__(self, real):
    self._real, self.launched = real, collections.Counter()

  def __getattr__(self, name):
    fn = getattr(self._real, name)
    if name not in mode_hip.LAUNCHING or name == 'mode_debug_poison':
      return fn

    def call(*args):
      self.launched[name] += 1
      return fn(*args)

    return call


Case = collections.namedtuple('Case', 'id name entries build args arith switches')
CASES = []
STATS = {'allocations': 0, 'launches': 0, 'cases': 0}  # what the run saw (printed by the last test of the module)
LAUNCHES = {  # case id -> the launching entries (without their mode_ prefix) that mode_hip.functional's routing takes it through
    'cost_volume-1x3x7x2x5':
        'cost_volume_bwd cost_volume_fwd',
    'cost_volume-2x4x6x5x16':
        'cost_volume_bwd cost_volume_fwd',
    'cost_conv-1x3x5x7x4x5':
        'cost_conv_assemble_bwd cost_conv_assemble_fwd cost_conv_assemble_fwd_bn cost_conv_assemble_fwd_bn_amax sphere_conv_bwd_data_adj sphere_conv_bwd_weight sphere_conv_fwd',
    'cost_conv-1x2x3x4x1x130':
        'cost_conv_assemble_bwd cost_conv_assemble_fwd cost_conv_assemble_fwd_bn cost_conv_assemble_fwd_bn_amax sphere_conv_bwd_data_adj sphere_conv_bwd_weight sphere_conv_fwd',
    'sphere_gather-ERPx10x20x1x5x7-f32':
        'sphere_conv_bwd_data_adj sphere_conv_bwd_weight sphere_conv_fwd sphere_conv_fwd_bn',
    'sphere_gather-ERPx16x32x2x4x6x2-f32':
        'sphere_conv_bwd_data_adj sphere_conv_bwd_weight sphere_conv_fwd sphere_conv_fwd_bn',
    'sphere_gather-Cassinix32x16x2x4x4x1x2-f32':
        'sphere_conv_bwd_data_adj sphere_conv_bwd_weight sphere_conv_fwd sphere_conv_fwd_win_bn transpose_planes',
    'sphere_gather-ERPx10x20x1x5x7-bf16x6':
        'sphere_conv_bwd_data_adj sphere_conv_bwd_weight sphere_conv_fwd sphere_conv_fwd_bn',
    'sphere_gather-ERPx16x32x2x4x6x2-bf16x6':
        'sphere_conv_bwd_data_adj sphere_conv_bwd_weight sphere_conv_fwd sphere_conv_fwd_bn',
    'sphere_gather-Cassinix32x16x2x4x4x1x2-bf16x6':
        'sphere_conv_bwd_data_adj sphere_conv_bwd_weight sphere_conv_fwd sphere_conv_fwd_win_split transpose_planes',
    'sphere_gather-ERPx16x32x1x40x160-bf16x6':
        'sphere_conv_bwd_data_adj sphere_conv_bwd_weight sphere_conv_fwd sphere_conv_fwd_bn',
    'sphere_gather_scatter-Cassinix32x16x2x4x4x1x2x3x3xgnomonicxFalsexFalsexTrue-f32':
        'sphere_conv_bwd_data sphere_conv_bwd_data_adj sphere_conv_bwd_weight sphere_conv_fwd sphere_conv_fwd_win_bn transpose_planes',
    'sphere_taps-ERPx16x32x2x6x10x1x1x1x3-bf16x6':
        'sphere_conv_bwd_data_adj sphere_conv_bwd_weight sphere_conv_fwd sphere_conv_fwd_bn',
    'sphere_taps-ERPx16x32x2x6x10x1x1x2x2-bf16x6':
        'sphere_conv_bwd_data_adj sphere_conv_bwd_weight sphere_conv_fwd',
    'sphere_taps-ERPx16x32x2x6x10x1x1x5x5-bf16x6':
        'sphere_conv_bwd_data_adj sphere_conv_bwd_weight sphere_conv_fwd sphere_conv_fwd_bn',
    'sphere_random_table--x24x20x1x6x8x1x1x3x3xrandom-bf16x6':
        'sphere_conv_bwd_data_adj sphere_conv_bwd_weight sphere_conv_fwd sphere_conv_fwd_bn',
    'sphere_window-Cassinix33x66x1x12x40x1x2-f32':
        'sphere_conv_bwd_data_adj sphere_conv_bwd_weight_win sphere_conv_fwd_win sphere_conv_fwd_win_bn transpose_planes',
    'sphere_window-Cassinix33x66x1x12x40x1x2-bf16x6':
        'abs_max sphere_conv_bwd_data_adj sphere_conv_bwd_weight_win_split_f16 sphere_conv_fwd_win_split transpose_planes',
    'sphere_window-Cassinix10x20x2x5x7-f32':
        'sphere_conv_bwd_data_adj sphere_conv_bwd_weight_win sphere_conv_fwd_win sphere_conv_fwd_win_bn transpose_planes',
    'sphere_window-Cassinix10x20x2x5x7-bf16x6':
        'abs_max sphere_conv_bwd_data_adj sphere_conv_bwd_weight_win_split_f16 sphere_conv_fwd_win_split transpose_planes',
    'sphere_window-Cassinix36x72x1x8x12x1x2-f32':
        'sphere_conv_bwd_data_adj sphere_conv_bwd_weight_win sphere_conv_fwd_win sphere_conv_fwd_win_bn transpose_planes',
    'sphere_window-Cassinix36x72x1x8x12x1x2-bf16x6':
        'abs_max sphere_conv_bwd_data_adj sphere_conv_bwd_weight_win_split_f16 sphere_conv_fwd_win_split transpose_planes',
    'sphere_window-Cassinix32x64x3x40x16-f32':
        'sphere_conv_bwd_data_adj sphere_conv_bwd_weight sphere_conv_fwd_win sphere_conv_fwd_win_bn transpose_planes',
    'sphere_window-Cassinix32x64x3x40x16-bf16x6':
        'sphere_conv_bwd_data_adj sphere_conv_bwd_weight sphere_conv_fwd_win_split transpose_planes',
    'sphere_window_nopolar-Cassinix33x66x1x12x40x1x2-bf16x6-SPHERE_POLAR=False':
        'abs_max sphere_conv_bwd_data_adj sphere_conv_bwd_weight_win_split_f16 sphere_conv_fwd_win_split transpose_planes',
    'sphere_window_nchw-Cassinix36x72x1x8x12x1x2-f32-SPHERE_LAYOUT=nchw':
        'sphere_conv_bwd_data_adj sphere_conv_bwd_weight_win sphere_conv_fwd_win sphere_conv_fwd_win_bn transpose_planes',
    'sphere_window_split-Cassinix32x64x2x16x32x1x1x3x3xgnomonicxTruexTrue-bf16x6-SPHERE_BWD_F16=True-SPHERE_FWD_F16=True':
        'abs_max sphere_conv_bwd_data_adj sphere_conv_bwd_data_win_split_f16 sphere_conv_bwd_weight sphere_conv_fwd_win_split sphere_conv_fwd_win_split_f16 transpose_planes',
    'sphere_window_split-Cassinix32x64x2x16x32x1x1x3x3xgnomonicxFalsexTrue-bf16x6-SPHERE_BWD_F16=False-SPHERE_FWD_F16=False':
        'sphere_conv_bwd_data_adj sphere_conv_bwd_data_win_split sphere_conv_bwd_weight sphere_conv_fwd_win_split transpose_planes',
    'sphere_window_split-Cassinix32x64x2x32x32x1x2x3x3xgnomonicxTruexTrue-bf16x6':
        'abs_max sphere_conv_bwd_data_adj sphere_conv_bwd_data_win_split_f16 sphere_conv_bwd_weight sphere_conv_fwd_win_split sphere_conv_fwd_win_split_f16 transpose_planes',
    'sphere_window_nosplit-Cassinix32x64x2x16x32x1x1x3x3xgnomonicxFalsexTrue-bf16x6-SPHERE_BWD_DATA_SPLIT=False-SPHERE_BWD_WEIGHT_SPLIT=False':
        'sphere_conv_bwd_data_adj sphere_conv_bwd_weight sphere_conv_fwd_win_split transpose_planes',
    'sphere_window_erp-ERPx33x66x1x12x40x1x2-f32':
        'sphere_conv_bwd_data_adj sphere_conv_bwd_weight_win sphere_conv_fwd_win sphere_conv_fwd_win_bn',
    'sphere_window_erp-ERPx33x66x1x12x40x1x2-bf16x6':
        'abs_max sphere_conv_bwd_data_adj sphere_conv_bwd_weight_win_split_f16 sphere_conv_fwd_win_split',
    'sphere_window_bf16-Cassinix33x66x1x12x40x1x2-bf16x6-SPHERE_BWD_F16=False-SPHERE_FWD_F16=False':
        'sphere_conv_bwd_data_adj sphere_conv_bwd_weight_win_split sphere_conv_fwd_win_split transpose_planes',
    'sphere_window_128x256-Cassinix128x256x1x48x32x1x2x3x3xgnomonicxTruexTrue-f32':
        'sphere_conv_bwd_data_adj sphere_conv_bwd_weight_win sphere_conv_fwd_win sphere_conv_fwd_win_bn transpose_planes',
    'sphere_window_128x256-Cassinix128x256x1x48x32x1x2x3x3xgnomonicxTruexTrue-bf16x6':
        'abs_max sphere_conv_bwd_data_adj sphere_conv_bwd_data_adj_list sphere_conv_bwd_data_win_split_f16 sphere_conv_bwd_weight_win_split_f16 sphere_conv_fwd_win_split transpose_planes',
    'conv3d_s1-2x16x20x5x7x33-f32':
        'conv3d_bwd_data conv3d_bwd_weight conv3d_fwd',
    'conv3d_s1-1x32x32x3x17x130-f32':
        'conv3d_bwd_data conv3d_bwd_weight conv3d_fwd',
    'conv3d_s1-2x8x8x8x8x8-f32':
        'conv3d_bwd_data conv3d_bwd_weight conv3d_fwd',
    'conv3d_s1_wgrad-2x20x40x5x7x33x1xFalsexwgrad-f32':
        'conv3d_bwd_weight',
    'conv3d_s1_wgrad-1x16x16x1x2x31x1xFalsexwgrad-f32':
        'conv3d_bwd_weight',
    'conv3d_s1_acc-1x64x64x4x9x33x1xFalsexacc-f32':
        'conv3d_bwd_data',
    'conv3d_s1_acc-1x24x40x4x6x34x1xFalsexacc-f32':
        'conv3d_bwd_data',
    'conv3d_head-1x20x1x3x5x33-f32':
        'conv3d_bwd_data conv3d_bwd_weight conv3d_fwd',
    'conv3d_head-2x32x1x1x1x7-f32':
        'conv3d_bwd_data conv3d_bwd_weight conv3d_fwd',
    'conv3d_s1-2x16x20x5x7x33-bf16x6':
        'abs_max conv3d_bwd_data conv3d_bwd_weight_split_f16 conv3d_fwd_split_f16',
    'conv3d_s1-1x32x32x3x17x130-bf16x6':
        'abs_max conv3d_bwd_data_split_f16 conv3d_bwd_weight_split_f16 conv3d_fwd_split_f16',
    'conv3d_s1-2x8x8x8x8x8-bf16x6':
        'abs_max conv3d_bwd_data_split_f16 conv3d_bwd_weight_split_f16 conv3d_fwd_split_f16',
    'conv3d_s1_wgrad-2x20x40x5x7x33x1xFalsexwgrad-bf16x6':
        'abs_max conv3d_bwd_weight_split_f16',
    'conv3d_s1_wgrad-1x16x16x1x2x31x1xFalsexwgrad-bf16x6':
        'abs_max conv3d_bwd_weight_split_f16',
    'conv3d_s1_acc-1x64x64x4x9x33x1xFalsexacc-bf16x6':
        'abs_max conv3d_bwd_data_split_f16',
    'conv3d_s1_acc-1x24x40x4x6x34x1xFalsexacc-bf16x6':
        'abs_max conv3d_bwd_data_split_f16',
    'conv3d_head-1x20x1x3x5x33-bf16x6':
        'conv3d_bwd_data conv3d_bwd_weight conv3d_fwd',
    'conv3d_head-2x32x1x1x1x7-bf16x6':
        'conv3d_bwd_data conv3d_bwd_weight conv3d_fwd',
    'conv3d_s1-2x16x20x5x7x33-bf16x6-CONV3D_S1_F16=False':
        'conv3d_bwd_data conv3d_bwd_weight_split conv3d_fwd_split',
    'conv3d_s1-1x32x32x3x17x130-bf16x6-CONV3D_S1_F16=False':
        'conv3d_bwd_data_split conv3d_bwd_weight_split conv3d_fwd_split',
    'conv3d_s1-2x8x8x8x8x8-bf16x6-CONV3D_S1_F16=False':
        'conv3d_bwd_data_split conv3d_bwd_weight_split conv3d_fwd_split',
    'conv3d_s1_wgrad-2x20x40x5x7x33x1xFalsexwgrad-bf16x6-CONV3D_S1_F16=False':
        'conv3d_bwd_weight_split',
    'conv3d_s1_wgrad-1x16x16x1x2x31x1xFalsexwgrad-bf16x6-CONV3D_S1_F16=False':
        'conv3d_bwd_weight_split',
    'conv3d_s1_acc-1x64x64x4x9x33x1xFalsexacc-bf16x6-CONV3D_S1_F16=False':
        'conv3d_bwd_data_split conv3d_bwd_data_split_acc',
    'conv3d_s1_acc-1x24x40x4x6x34x1xFalsexacc-bf16x6-CONV3D_S1_F16=False':
        'conv3d_bwd_data_split conv3d_bwd_data_split_acc',
    'conv3d_head-1x20x1x3x5x33-bf16x6-CONV3D_S1_F16=False':
        'conv3d_bwd_data conv3d_bwd_weight conv3d_fwd',
    'conv3d_head-2x32x1x1x1x7-bf16x6-CONV3D_S1_F16=False':
        'conv3d_bwd_data conv3d_bwd_weight conv3d_fwd',
    'conv3d_s2-2x20x40x4x6x70x2-f32':
        'conv3d_bwd_data conv3d_bwd_weight conv3d_fwd',
    'conv3d_s2-1x32x64x4x8x64x2-f32':
        'conv3d_bwd_data conv3d_bwd_weight conv3d_fwd',
    'conv3d_s2_wgrad-1x64x64x6x8x24x2xFalsexwgrad-f32':
        'conv3d_bwd_weight',
    'conv3d_s2_wgrad-3x64x128x2x4x8x2xFalsexwgrad-f32':
        'conv3d_bwd_weight',
    'conv3d_s2_acc-1x64x64x4x8x34x2xFalsexacc-f32':
        'conv3d_bwd_data',
    'conv3d_s2_acc-1x40x24x4x6x34x2xFalsexacc-f32':
        'conv3d_bwd_data',
    'deconv3d-2x24x40x2x5x35x2xTrue-f32':
        'conv3d_bwd_weight conv3d_fwd deconv3d_fwd',
    'deconv3d-1x64x32x6x16x32x2xTrue-f32':
        'conv3d_bwd_weight conv3d_fwd deconv3d_fwd',
    'deconv3d-2x12x40x3x5x34x2xTrue-f32':
        'conv3d_bwd_weight conv3d_fwd deconv3d_fwd',
    'deconv3d-2x20x8x3x5x34x2xTrue-f32':
        'conv3d_bwd_weight conv3d_fwd deconv3d_fwd',
    'conv3d_s2-2x20x40x4x6x70x2-bf16x6':
        'conv3d_bwd_data_s2_split conv3d_bwd_weight conv3d_fwd',
    'conv3d_s2-1x32x64x4x8x64x2-bf16x6':
        'conv3d_bwd_data_s2_split conv3d_bwd_weight_s2_split conv3d_fwd_s2_split',
    'conv3d_s2_wgrad-1x64x64x6x8x24x2xFalsexwgrad-bf16x6':
        'conv3d_bwd_weight_s2_split',
    'conv3d_s2_wgrad-3x64x128x2x4x8x2xFalsexwgrad-bf16x6':
        'conv3d_bwd_weight_s2_split',
    'conv3d_s2_acc-1x64x64x4x8x34x2xFalsexacc-bf16x6':
        'conv3d_bwd_data_s2_split conv3d_bwd_data_split_acc',
    'conv3d_s2_acc-1x40x24x4x6x34x2xFalsexacc-bf16x6':
        'conv3d_bwd_data_s2_split',
    'deconv3d-2x24x40x2x5x35x2xTrue-bf16x6':
        'conv3d_bwd_weight conv3d_fwd deconv3d_fwd_split',
    'deconv3d-1x64x32x6x16x32x2xTrue-bf16x6':
        'conv3d_bwd_weight_s2_split conv3d_fwd_s2_split deconv3d_fwd_split',
    'deconv3d-2x12x40x3x5x34x2xTrue-bf16x6':
        'conv3d_bwd_weight conv3d_fwd deconv3d_fwd',
    'deconv3d-2x20x8x3x5x34x2xTrue-bf16x6':
        'conv3d_bwd_weight conv3d_fwd deconv3d_fwd',
    'conv3d_bn_eval-20x40x1xFalse-f32':
        'conv3d_fwd_bn',
    'conv3d_bn_eval-64x64x1xFalse-f32':
        'conv3d_fwd_bn',
    'conv3d_bn_eval-32x64x2xFalse-f32':
        'conv3d_fwd_bn',
    'deconv3d_bn_eval-64x32x2xTrue-f32':
        'deconv3d_fwd_bn',
    'conv3d_bn_eval-20x40x1xFalse-bf16x6':
        'conv3d_fwd_bn',
    'conv3d_bn_eval-64x64x1xFalse-bf16x6':
        'abs_max conv3d_fwd_split_f16_bn',
    'conv3d_bn_eval-32x64x2xFalse-bf16x6':
        'conv3d_fwd_s2_split_amax',
    'deconv3d_bn_eval-64x32x2xTrue-bf16x6':
        'deconv3d_fwd_split_bn deconv3d_fwd_split_bn_amax',
    'conv3d_bn_eval-20x40x1xFalse-bf16x6-CONV3D_EVAL_F16=False':
        'conv3d_fwd_bn',
    'conv3d_bn_eval-64x64x1xFalse-bf16x6-CONV3D_EVAL_F16=False':
        'conv3d_fwd_split',
    'conv3d_bn_eval-32x64x2xFalse-bf16x6-CONV3D_EVAL_F16=False':
        'conv3d_fwd_s2_split_amax',
    'deconv3d_bn_eval-64x32x2xTrue-bf16x6-CONV3D_EVAL_F16=False':
        'deconv3d_fwd_split_bn deconv3d_fwd_split_bn_amax',
    'conv3d_bn_eval-16x24x2xFalse-f32':
        'conv3d_fwd_bn',
    'deconv3d_bn_eval-12x40x2xTrue-f32':
        'deconv3d_fwd_bn',
    'deconv3d_bn_eval-24x40x2xTrue-f32':
        'deconv3d_fwd_bn',
    'deconv3d_bn_eval-20x8x2xTrue-f32':
        'deconv3d_fwd_bn',
    'conv3d_bn_eval-16x24x2xFalse-bf16x6':
        'conv3d_fwd_bn',
    'deconv3d_bn_eval-12x40x2xTrue-bf16x6':
        'deconv3d_fwd_bn',
    'deconv3d_bn_eval-24x40x2xTrue-bf16x6':
        'deconv3d_fwd_bn',
    'deconv3d_bn_eval-20x8x2xTrue-bf16x6':
        'deconv3d_fwd_bn',
    'conv3d_stats-1x32x64x5x9x33xTruexFalse-bf16x6-CONV3D_BN_STATS=True':
        'abs_max bn_train_bwd bn_train_bwd_amax bn_train_fwd_prestats bn_train_fwd_prestats_amax conv3d_bwd_data_split_f16 conv3d_bwd_weight_split_f16 conv3d_fwd_split_stats',
    'conv3d_stats-1x32x64x5x9x33xFalsexTrue-bf16x6-CONV3D_BN_STATS=True':
        'abs_max bn_train_bwd bn_train_bwd_amax bn_train_fwd_prestats bn_train_fwd_prestats_amax conv3d_bwd_data_split_f16 conv3d_bwd_weight_split_f16 conv3d_fwd_split_stats',
    'conv2d_3x3-2x20x40x7x33x1-f32':
        'conv2d_bwd_data conv2d_bwd_weight conv2d_fwd conv2d_fwd_bn',
    'conv2d_3x3-1x8x8x3x5x2-f32':
        'conv2d_bwd_data conv2d_bwd_weight conv2d_fwd conv2d_fwd_bn',
    'conv2d_3x3-1x16x40x9x31x2-f32':
        'conv2d_bwd_data conv2d_bwd_weight conv2d_fwd conv2d_fwd_bn',
    'conv2d_3x3-1x32x64x9x33x2-f32':
        'conv2d_bwd_data conv2d_bwd_weight conv2d_fwd conv2d_fwd_bn',
    'conv2d_3x3-2x20x40x7x33x1-bf16x6':
        'abs_max conv2d_bwd_data conv2d_bwd_weight_split_f16 conv2d_fwd conv2d_fwd_bn',
    'conv2d_3x3-1x8x8x3x5x2-bf16x6':
        'abs_max conv2d_bwd_data conv2d_bwd_weight_split_f16 conv2d_fwd conv2d_fwd_bn',
    'conv2d_3x3-1x16x40x9x31x2-bf16x6':
        'abs_max conv2d_bwd_data conv2d_bwd_weight_split_f16 conv2d_fwd_split conv2d_fwd_split_f16 conv2d_fwd_split_f16_bn',
    'conv2d_3x3-1x32x64x9x33x2-bf16x6':
        'abs_max conv2d_bwd_data_split conv2d_bwd_data_split_acc conv2d_bwd_data_split_f16 conv2d_bwd_weight_split_f16 conv2d_fwd_split conv2d_fwd_split_f16 conv2d_fwd_split_f16_bn',
    'conv2d_3x3-2x20x40x7x33x1-bf16x6-CONV2D_EVAL_F16=False-CONV2D_F16=False':
        'conv2d_bwd_data conv2d_bwd_weight_split conv2d_fwd conv2d_fwd_bn',
    'conv2d_3x3-1x8x8x3x5x2-bf16x6-CONV2D_EVAL_F16=False-CONV2D_F16=False':
        'conv2d_bwd_data conv2d_bwd_weight_split conv2d_fwd conv2d_fwd_bn',
    'conv2d_3x3-1x16x40x9x31x2-bf16x6-CONV2D_EVAL_F16=False-CONV2D_F16=False':
        'conv2d_bwd_data conv2d_bwd_weight_split conv2d_fwd_split',
    'conv2d_3x3-1x32x64x9x33x2-bf16x6-CONV2D_EVAL_F16=False-CONV2D_F16=False':
        'conv2d_bwd_data_split conv2d_bwd_data_split_acc conv2d_bwd_weight_split conv2d_fwd_split',
    'conv1x1-1x5x7x3x12x1x1x0-bf16x6':
        'conv1x1_bwd_data conv1x1_bwd_weight conv1x1_fwd conv1x1_fwd_bn',
    'conv1x1-2x12x200x6x8x1x1x0-bf16x6':
        'conv1x1_bwd_data conv1x1_bwd_weight conv1x1_fwd conv1x1_fwd_bn',
    'conv1x1-1x10x6x6x16x1x2x0-bf16x6':
        'conv1x1_bwd_data conv1x1_bwd_weight conv1x1_fwd conv1x1_fwd_bn',
    'conv1x1-2x16x24x7x16x1x2x0-bf16x6':
        'conv1x1_bwd_data conv1x1_bwd_weight conv1x1_fwd conv1x1_fwd_bn',
    'conv1x1-2x8x8x16x24x1x2x0-bf16x6':
        'conv1x1_bwd_data conv1x1_bwd_weight conv1x1_fwd conv1x1_fwd_bn',
    'conv_stem-2x3x20x26x70x7x2x3xFalse-bf16x6':
        'conv_stem_bwd_weight conv_stem_fwd conv_stem_fwd_bn',
    'conv_stem-1x3x32x8x8x7x2x3xFalse-bf16x6':
        'conv_stem_bwd_weight conv_stem_fwd conv_stem_fwd_bn',
    'conv2d_3x3_s2-2x8x8x2x4x3x2x1-f32':
        'bn_eval_fwd conv2d_bwd_data conv2d_bwd_weight sphere_conv_fwd zero_insert2',
    'conv2d_3x3_s2-1x20x40x10x36x3x2x1-f32':
        'conv2d_bwd_data conv2d_bwd_weight sphere_conv_fwd sphere_conv_fwd_bn zero_insert2',
    'conv2d_3x3_s2-2x8x8x2x4x3x2x1-bf16x6':
        'abs_max bn_eval_fwd conv2d_bwd_data conv2d_bwd_weight_split_f16 sphere_conv_fwd zero_insert2',
    'conv2d_3x3_s2-1x20x40x10x36x3x2x1-bf16x6':
        'abs_max conv2d_bwd_data conv2d_bwd_weight_split_f16 sphere_conv_fwd sphere_conv_fwd_bn zero_insert2',
    'conv2d_tabled-1x5x7x9x11x3x2x1-bf16x6':
        'sphere_conv_bwd_data_adj sphere_conv_bwd_weight sphere_conv_fwd sphere_conv_fwd_bn',
    'conv2d_tabled-1x6x4x10x13x5x3x2-bf16x6':
        'sphere_conv_bwd_data_adj sphere_conv_bwd_weight sphere_conv_fwd sphere_conv_fwd_bn',
    'bn_act-(3,5,2,2,4)xTruexFalse-bf16x6':
        'bn_eval_fwd bn_train_bwd bn_train_bwd_amax bn_train_fwd bn_train_fwd_amax',
    'bn_act-(2,6,3,5,7)xTruexFalse-bf16x6':
        'bn_eval_fwd bn_train_bwd bn_train_bwd_amax bn_train_fwd bn_train_fwd_amax',
    'bn_act-(2,16,9,11)xTruexFalse-bf16x6':
        'bn_eval_fwd bn_train_bwd bn_train_bwd_amax bn_train_fwd bn_train_fwd_amax',
    'bn_act_groups-(4,6,7,9)xTruexFalsex2-bf16x6':
        'bn_eval_fwd bn_train_bwd bn_train_bwd_amax bn_train_fwd bn_train_fwd_amax',
    'bn_act-(3,5,2,2,4)xFalsexTrue-bf16x6':
        'bn_eval_fwd bn_train_bwd bn_train_bwd_amax bn_train_fwd bn_train_fwd_amax',
    'bn_act-(2,6,3,5,7)xFalsexTrue-bf16x6':
        'bn_eval_fwd bn_train_bwd bn_train_bwd_amax bn_train_fwd bn_train_fwd_amax',
    'bn_act-(2,16,9,11)xFalsexTrue-bf16x6':
        'bn_eval_fwd bn_train_bwd bn_train_bwd_amax bn_train_fwd bn_train_fwd_amax',
    'bn_act_groups-(4,6,7,9)xFalsexTruex2-bf16x6':
        'bn_eval_fwd bn_train_bwd bn_train_bwd_amax bn_train_fwd bn_train_fwd_amax',
    'bn_act-(3,5,2,2,4)xTruexTrue-bf16x6':
        'bn_eval_fwd bn_train_bwd bn_train_bwd_amax bn_train_fwd bn_train_fwd_amax',
    'bn_act-(2,6,3,5,7)xTruexTrue-bf16x6':
        'bn_eval_fwd bn_train_bwd bn_train_bwd_amax bn_train_fwd bn_train_fwd_amax',
    'bn_act-(2,16,9,11)xTruexTrue-bf16x6':
        'bn_eval_fwd bn_train_bwd bn_train_bwd_amax bn_train_fwd bn_train_fwd_amax',
    'bn_act_groups-(4,6,7,9)xTruexTruex2-bf16x6':
        'bn_eval_fwd bn_train_bwd bn_train_bwd_amax bn_train_fwd bn_train_fwd_amax',
    'bn_act-(3,5,2,2,4)xFalsexFalse-bf16x6':
        'bn_eval_fwd bn_train_bwd bn_train_bwd_amax bn_train_fwd bn_train_fwd_amax',
    'bn_act-(2,6,3,5,7)xFalsexFalse-bf16x6':
        'bn_eval_fwd bn_train_bwd bn_train_bwd_amax bn_train_fwd bn_train_fwd_amax',
    'bn_act-(2,16,9,11)xFalsexFalse-bf16x6':
        'bn_eval_fwd bn_train_bwd bn_train_bwd_amax bn_train_fwd bn_train_fwd_amax',
    'bn_act_groups-(4,6,7,9)xFalsexFalsex2-bf16x6':
        'bn_eval_fwd bn_train_bwd bn_train_bwd_amax bn_train_fwd bn_train_fwd_amax',
    'bn_act-(2,6,3,5,7)xTruexTrue-f32':
        'bn_eval_fwd bn_train_bwd bn_train_bwd_amax bn_train_fwd bn_train_fwd_amax',
    'classif_head-2x5x(5,11,37)xTrue-f32':
        'classif_train_bwd classif_train_bwd_amax classif_train_fwd',
    'classif_head-1x32x(13,20,70)xTrue-f32':
        'classif_train_bwd classif_train_bwd_amax classif_train_fwd',
    'classif_head-2x5x(5,11,37)xTrue-bf16x6':
        'classif_train_bwd classif_train_bwd_amax classif_train_fwd',
    'classif_head-1x32x(13,20,70)xTrue-bf16x6':
        'classif_train_bwd classif_train_bwd_amax classif_train_fwd',
    'head-1x12x5x7x4':
        'head_bwd head_fwd',
    'head-1x3x4x4x3':
        'head_bwd head_fwd',
    'head_two_kernel_bwd-1x4x2x100x(16,8,512)':
        'head_bwd head_fwd',
    'head_loss-2x4x16x8':
        'head_bwd_loss head_fwd smooth_l1_masked',
    'small_ops-1':
        'abs_max abs_max_batch sum_n',
    'small_ops-1023':
        'abs_max abs_max_batch sum_n',
    'small_ops-4097':
        'abs_max abs_max_batch sum_n',
    'planes':
        'transpose_planes zero_insert2',
    'maxpool2x2-(1,3,9,7)':
        'maxpool2x2_bwd maxpool2x2_fwd',
    'maxpool2x2-(1,2,2,2)':
        'maxpool2x2_bwd maxpool2x2_fwd',
    'deconv2x2-2x16x8x6x8':
        'conv1x1_bwd_data conv1x1_bwd_weight conv1x1_fwd depth_to_space2 space_to_depth2',
    'conv1x1_sigmoid-1x8x6x10':
        'conv1x1_sigmoid_bwd conv1x1_sigmoid_fwd',
    'metrics-1':
        'masked_metrics silog_loss_bwd silog_loss_fwd',
    'metrics-1023':
        'masked_metrics silog_loss_bwd silog_loss_fwd',
    'metrics-4097':
        'masked_metrics silog_loss_bwd silog_loss_fwd',
    'erp_metrics-50x25x1':
        'bicubic_up2 erp_depth_metrics',
    'erp_metrics-50x25x3':
        'bicubic_up2 erp_depth_metrics',
    'erp_metrics-26x13x3':
        'bicubic_up2 erp_depth_metrics',
    'geometry':
        'depth_view_project depth_view_trans disp2depth grid_sample_border zbuffer',
    'multiview-1':
        'depth_view_trans disp2depth grid_sample_border multiview_handoff',
    'multiview-3':
        'depth_view_trans disp2depth grid_sample_border multiview_handoff',
    'path_train_step':
        'abs_max abs_max_batch bn_train_bwd_amax bn_train_fwd_amax classif_train_bwd_amax classif_train_fwd conv1x1_bwd_data conv1x1_bwd_weight conv1x1_fwd conv2d_bwd_data_split_f16 conv2d_bwd_weight_split_f16 conv2d_fwd_split_f16 conv3d_bwd_data_s2_split conv3d_bwd_data_split_acc conv3d_bwd_data_split_f16 conv3d_bwd_weight_s2_split conv3d_bwd_weight_split_f16 conv3d_fwd_s2_split conv3d_fwd_split_f16 conv_stem_bwd_weight conv_stem_fwd cost_conv_assemble_bwd cost_conv_assemble_fwd deconv3d_fwd_split head_bwd head_fwd sphere_conv_bwd_data_adj sphere_conv_bwd_weight sphere_conv_bwd_weight_win_split_f16 sphere_conv_fwd sum_n transpose_planes zero_insert2',
    'path_eval_forward':
        'abs_max bn_train_fwd_amax conv1x1_fwd conv1x1_fwd_bn conv2d_fwd_split conv2d_fwd_split_f16_bn conv3d_fwd conv3d_fwd_s2_split conv3d_fwd_s2_split_amax conv3d_fwd_split_f16 conv3d_fwd_split_f16_bn conv_stem_fwd conv_stem_fwd_bn cost_conv_assemble_fwd cost_conv_assemble_fwd_bn_amax deconv3d_fwd_split deconv3d_fwd_split_bn_amax head_fwd sphere_conv_fwd sphere_conv_fwd_bn',
    'path_fusion':
        'abs_max bn_train_bwd_amax bn_train_fwd_amax conv1x1_bwd_data conv1x1_bwd_weight conv1x1_fwd conv1x1_sigmoid_bwd conv1x1_sigmoid_fwd conv2d_bwd_data conv2d_bwd_data_split_f16 conv2d_bwd_weight_split_f16 conv2d_fwd conv2d_fwd_bn conv2d_fwd_split_f16 conv2d_fwd_split_f16_bn depth_to_space2 maxpool2x2_bwd maxpool2x2_fwd space_to_depth2',
    'sphere_gather-ERPx16x32x1x40x160-f32':
        'sphere_conv_bwd_data_adj sphere_conv_bwd_weight sphere_conv_fwd sphere_conv_fwd_bn',
    'sphere_window_128x256-Cassinix128x256x1x48x32x1x2x3x3xgnomonicxTruexTrue-bf16x6-SPHERE_POLAR=False':
        'abs_max sphere_conv_bwd_data_adj sphere_conv_bwd_data_adj_list sphere_conv_bwd_data_win_split_f16 sphere_conv_bwd_weight_win_split_f16 sphere_conv_fwd_win_split transpose_planes',
}
LAUNCHES = {k: tuple('mode_' + e for e in v.split()) for k, v in LAUNCHES.items()}


_IN_THE_NAME = ('SPHERE_FWD', 'SPHERE_BWD_WEIGHT', 'SPHERE_FWD_MIN_WG', 'SPHERE_BWD_SPLIT_MIN_WG')  # switches the case's name stands for


def _id(name, args, arith, switches):
  bits = [name] + ['x'.join(str(a) for a in args).replace(' ', '')] * bool(args) + [arith] * bool(arith)
  return '-'.join(bits + ['%s=%s' % (k, v) for k, v in sorted(switches.items()) if k not in _IN_THE_NAME])


def case(name, entries, build, args=(), arith=None, **switches):
  """Register one case.  build(*args) -> (run, verify): run() makes FRESH placed inputs, launches, returns {name: tensor};
  verify(out) compares the first fill's outputs ({name: CPU tensor}) with float64.  arith: HF.set_conv_arith; switches: HF attributes.
  entries: the launching C-ABI entries the case is there for; the routing of mode_hip.functional adds those of LAUNCHES[id]."""
  cid = _id(name, args, arith, switches)
  assert cid not in [c.id for c in CASES], cid
  CASES.append(Case(cid, name, frozenset(entries) | frozenset(LAUNCHES.get(cid, ())), build, tuple(args), arith, switches))


def _rand(shape, seed, scale=1.0):
  return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32))


def P(t):
  """A CPU tensor -> a guarded device copy."""
  return GB.place(t.to(DEV))


def _fresh_caches():
  """Plans, adjoints, packs and tables are cached on (data_ptr, _version) or on the geometry: drop them, so that every run allocates
  them inside its own guarded context."""
  from models.basic.spherical_conv import sphere_conv as SC
  from utils import geometry as UG
  for c in (HF._plan_cache, HF._adjoint_cache, HF._pos_t_cache, HF._adjplan_cache, HF._conv_tables, UG._frames_cache):
    c.d.clear()
    c.pinned.clear()
  SC._device_tables.clear()
  for v in vars(UG).values():
    if hasattr(v, 'cache_clear'):
      v.cache_clear()


def close(out, name, want, tol, scale=True):
  """|out[name] - want| <= tol x max(1, |want|max) (scale) or <= tol."""
  got = out[name].double()
  assert tuple(got.shape) == tuple(want.shape), (name, got.shape, want.shape)
  err = float((got - want.detach().double()).abs().max())
  bound = tol * (max(1.0, float(want.abs().max())) if scale else 1.0)
  print('  %s: max err %.3e (bound %.3e)' % (name, err, bound))
  assert err <= bound, (name, err, bound)



def PO(t):
  """A buffer the operator writes (it may start as NaN): guarded, not counted as an input."""
  return GB.place(t.to(DEV), is_input=False)


class PlainTwins(object):
  """Library stand-in that turns a call of an `_amax` entry into a call of its plain twin: the same arguments minus the maximum's
  pointer (the entries the host code no longer calls -- the BatchNorm training passes, the folded cost_conv assembly, and likewise the
  classifier head's backward and the transposed split convolution's folded form: INTEGRATION.md offers them to outside binders)."""
  MAP = {'mode_bn_train_fwd_amax': ('mode_bn_train_fwd', -2), 'mode_bn_train_bwd_amax': ('mode_bn_train_bwd', -2),
         'mode_bn_train_fwd_prestats_amax': ('mode_bn_train_fwd_prestats', -2),
         'mode_cost_conv_assemble_fwd_bn_amax': ('mode_cost_conv_assemble_fwd_bn', 4),
         'mode_classif_train_bwd_amax': ('mode_classif_train_bwd', -2), 'mode_deconv3d_fwd_split_bn_amax': ('mode_deconv3d_fwd_split_bn', 4)}

  def __init__(self):
    self._real = mode_hip._lib

  def __getattr__(self, name):
    if name not in self.MAP:
      return getattr(self._real, name)
    plain, drop = self.MAP[name]
    fn = getattr(self._real, plain)

    def call(*args):
      args = list(args)
      del args[drop]
      return fn(*args)

    return call

  def __enter__(self):
    mode_hip._lib = self
    return self

  def __exit__(self, *exc):
    mode_hip._lib = self._real
    return False


def _bn_eval_module(C, seed, dims=3):
  """test_gpu_kernels._eval_bn with the four vectors in guarded views."""
  bn = (nn.BatchNorm3d if dims == 3 else nn.BatchNorm2d)(C).to(DEV).eval()
  bn.weight.data = P(_rand((C,), seed) * 0.2 + 1.0)
  bn.bias.data = P(_rand((C,), seed + 1) * 0.3)
  bn.running_mean.data = P(_rand((C,), seed + 2) * 0.5)
  bn.running_var.data = P(_rand((C,), seed + 3).abs() + 0.3)
  return bn


def _unfused(C, seed, y, add, relu, eps=1e-5):
  """float64 eval BatchNorm (+ add) (+ ReLU) of test_gpu_kernels._unfused, from the seeds of _bn_eval_module."""
  g, b = (_rand((C,), seed) * 0.2 + 1.0).double(), (_rand((C,), seed + 1) * 0.3).double()
  m, v = (_rand((C,), seed + 2) * 0.5).double(), (_rand((C,), seed + 3).abs() + 0.3).double()
  y = F.batch_norm(y.double(), m, v, g, b, False, 0.0, eps)
  if add is not None:
    y = y + add.double()
  return torch.relu(y) if relu else y


FOLD_VARIANTS = [(True, False), (False, True), (True, True), (False, False)]  # (relu, with_add) of test_gpu_kernels


# ============================================================================================================ cost volume, cost_conv
def b_cost_volume(B, C, D4, H, W):
  from oracle import mode_ref
  ref, tgt, g = _rand((B, C, H, W), 1), _rand((B, C, H, W), 2), _rand((B, 2 * C, D4, H, W), 4)

  def run():
    r, t = P(ref).requires_grad_(True), P(tgt).requires_grad_(True)
    cost = HF.cost_volume(r, t, D4)
    cost.backward(P(g))
    return {'cost': cost.detach(), 'g_ref': r.grad, 'g_tgt': t.grad}

  def verify(out):  # test_cost_volume_fwd_bit_exact, test_cost_volume_bwd
    ra, ta = ref.clone().requires_grad_(True), tgt.clone().requires_grad_(True)
    want = mode_ref.cost_volume(ra, ta, D4)
    want.backward(g)
    assert torch.equal(out['cost'], want.detach())
    assert torch.allclose(out['g_ref'], ra.grad, rtol=1e-5, atol=1e-5) and torch.allclose(out['g_tgt'], ta.grad, rtol=1e-5, atol=1e-5)

  return run, verify


for _a in ((1, 3, 7, 2, 5), (2, 4, 6, 5, 16)):
  case('cost_volume', ['mode_cost_volume_fwd', 'mode_cost_volume_bwd'], b_cost_volume, _a)


def b_cost_conv(B, C, Co, D4, H, W):
  from oracle import mode_ref
  ref, tgt = _rand((B, C, H, W), 31), _rand((B, C, H, W), 32)
  w, gy = _rand((Co, 2 * C, 3, 3, 3), 33, 0.2), _rand((B, Co, D4, H, W), 34)
  w_e = _rand((Co, 2 * C, 3, 3, 3), 111, 0.1)

  def run():
    rd, td, wd = P(ref).requires_grad_(True), P(tgt).requires_grad_(True), P(w).requires_grad_(True)
    y = HF.cost_conv(rd, td, wd, D4)
    y.backward(P(gy))
    out = {'y': y.detach(), 'g_ref': rd.grad, 'g_tgt': td.grad, 'g_w': wd.grad}
    with torch.no_grad():
      for relu in (True, False):
        r2, t2, w2 = P(ref), P(tgt), P(w_e)
        out['eval%d' % relu] = HF.cost_conv_bn_eval(r2, t2, w2, D4, _bn_eval_module(Co, 112), relu)
        with PlainTwins():
          out['plain%d' % relu] = HF.cost_conv_bn_eval(r2, t2, w2, D4, _bn_eval_module(Co, 112), relu)
    return out

  def verify(out):  # test_cost_conv_equals_conv3d_of_the_cost_volume, test_folded_batchnorm_cost_conv
    ra, ta, wa = ref.double().requires_grad_(True), tgt.double().requires_grad_(True), w.double().requires_grad_(True)
    y_ref = F.conv3d(mode_ref.cost_volume(ra, ta, D4), wa, None, 1, 1)
    y_ref.backward(gy.double())
    close(out, 'y', y_ref, 2e-6 * (2 * C * 27))
    for k, want in (('g_ref', ra.grad), ('g_tgt', ta.grad), ('g_w', wa.grad)):
      close(out, k, want, 1e-5)
    want = F.conv3d(mode_ref.cost_volume(ref.double(), tgt.double(), D4), w_e.double(), None, 1, 1)
    for relu in (True, False):
      close(out, 'eval%d' % relu, _unfused(Co, 112, want, None, relu), 1e-4, scale=False)
      assert torch.equal(out['plain%d' % relu], out['eval%d' % relu]), 'mode_cost_conv_assemble_fwd_bn equals its _amax twin bit for bit'

  return run, verify


for _a in ((1, 3, 5, 7, 4, 5), (1, 2, 3, 4, 1, 130)):
  case('cost_conv', ['mode_cost_conv_assemble_fwd', 'mode_cost_conv_assemble_bwd', 'mode_cost_conv_assemble_fwd_bn',
                     'mode_cost_conv_assemble_fwd_bn_amax'], b_cost_conv, _a)


# ============================================================================================================ spherical convolution
@functools.lru_cache(maxsize=None)
def _sphere_reference(typ, ih, iw, B, ci, co, stride, groups, kh, kw, table):
  from oracle import mode_ref, sphere_conv_ref
  if table == 'random':  # test_sphere_conv_unplannable_table_takes_the_gather_kernels
    g = torch.Generator().manual_seed(3)
    pos = torch.stack([torch.rand(9, ih, iw, generator=g) * (ih + 1) - 1, torch.rand(9, ih, iw, generator=g) * (iw + 1) - 1], 1).reshape(1, 18, ih, iw)
  else:
    pos = mode_ref.sphere_position(ih, iw, typ, (kh, kw)) if (kh, kw) != (3, 3) else mode_ref.sphere_position(ih, iw, typ)
  pos = pos.contiguous()
  H, W = pos.shape[2:]
  ph, pw = (kh - 1) // 2, (kw - 1) // 2
  Ho, Wo = sphere_conv_ref.out_size(H, kh, stride, ph, 1), sphere_conv_ref.out_size(W, kw, stride, pw, 1)
  x, w, gy = _rand((B, ci, H, W), 11), _rand((co, ci // groups, kh, kw), 12, 0.2), _rand((B, co, Ho, Wo), 13)
  cfg = ((stride, stride), (ph, pw), (1, 1), groups)
  y = sphere_conv_ref.forward(x.double(), pos, w.double(), *cfg)
  gx, gw = sphere_conv_ref.backward(x.double(), pos, w.double(), gy.double(), *cfg)
  return pos, x, w, gy, y, gx, gw


def b_sphere(typ, ih, iw, B, ci, co, stride=1, groups=1, kh=3, kw=3, table='gnomonic', f16=False, transposed_gy=False, scatter=False):
  """sphere_conv_fwd / _bwd_data / _bwd_weight and the folded-BatchNorm forward through HF, whatever kernels the switches select."""
  pos, x, w, gy, y_ref, gx_ref, gw_ref = _sphere_reference(typ, ih, iw, B, ci, co, stride, groups, kh, kw, table)
  st = (stride, stride)
  add = _rand(tuple(y_ref.shape), 108)
  same = tuple(y_ref.shape[2:]) == ((x.shape[2] - 1) // stride + 1, (x.shape[3] - 1) // stride + 1)  # (2 x 2 taps without padding: no folded form)

  def run():
    _fresh_caches()
    xd, wd, pd, gyd = P(x), P(w), P(pos), P(gy)
    y = PO(torch.full(tuple(y_ref.shape), float('nan')))
    HF.sphere_conv_fwd(xd, pd, wd, y, st, groups, f16=f16)
    out = {'y': y}
    gx = PO(torch.zeros(x.shape))
    HF.sphere_conv_bwd_data(gyd, pd, wd, gx, st, groups)
    out['gx'] = gx
    if stride == 1 and (kh, kw) == (3, 3):
      gxo = PO(torch.full(x.shape, float('nan')))
      HF.sphere_conv_bwd_data(gyd, pd, wd, gxo, st, groups, overwrite=True, gy_transposed=HF.transpose_planes(gyd) if transposed_gy else None)
      out['gx_overwrite'] = gxo
    if scatter:  # test_sphere_conv_bwd_data_scatter_form_matches_gather_form: the atomic form, straight through the ABI
      gs = PO(torch.zeros(x.shape))
      wp = HF._wpack(wd, groups)
      dims = HF._sc_dims(xd.shape, wd.shape, gyd.shape[2:], st, groups)
      mode_hip.check(mode_hip.lib().mode_sphere_conv_bwd_data(mode_hip.ptr(gyd), mode_hip.ptr(pd), mode_hip.ptr(wd), mode_hip.ptr(gs), mode_hip.ptr(wp),
                                                               *dims, mode_hip.stream_of(gyd)), 'mode_sphere_conv_bwd_data')
      # (float atomics: the one operator that is NOT bit-repeatable, DESIGN section 3 -- so not its bits but two verdicts are returned)
      out['scatter_finite'] = torch.isfinite(gs).all()
      out['scatter_close'] = (gs - gx).abs().max() < 1e-4 * max(1.0, float(gx.abs().max()))
    gw = PO(torch.zeros(w.shape))
    HF.sphere_conv_bwd_weight(gyd, pd, xd, gw, st, groups)
    out['gw'] = gw
    with torch.no_grad():
      for relu, with_add in ((True, True), (False, False)) if same else ():
        out['bn%d%d' % (relu, with_add)] = HF.sphere_conv_bn_eval(xd, pd, wd, _bn_eval_module(co, 107, 2), st, groups, P(add) if with_add else None, relu)
    return out

  def verify(out):
    k9 = (kh, kw) == (3, 3) and table == 'gnomonic'
    # test_sphere_conv_fwd_bwd / _window_kernels_match_gather_kernels; other tap counts and the random table: test_sphere_conv_other_kernel_sizes
    close(out, 'y', y_ref, 2e-6 * (ci // groups * 9) if k9 else 1e-4, scale=k9)
    close(out, 'gx', gx_ref, 2e-6 * (co * 9) if k9 else 1e-4, scale=k9)
    if 'gx_overwrite' in out:
      close(out, 'gx_overwrite', gx_ref, 1e-5 if k9 else 1e-4, scale=k9)  # test_sphere_conv_bwd_data_on_transposed_storage
    if 'scatter_close' in out:
      assert bool(out['scatter_finite']) and bool(out['scatter_close'])
    close(out, 'gw', gw_ref, 1e-5 if k9 else 1e-3, scale=k9)
    for relu, with_add in ((True, True), (False, False)) if same else ():  # test_folded_batchnorm_sphere_conv
      close(out, 'bn%d%d' % (relu, with_add), _unfused(co, 107, y_ref, add if with_add else None, relu), 1e-4, scale=False)

  return run, verify


GATHER = dict(SPHERE_FWD='gather', SPHERE_BWD_WEIGHT='gather', SPHERE_FWD_MIN_WG=0)
for _arith in ('f32', 'bf16x6'):
  case('sphere_gather', [], b_sphere, ('ERP', 10, 20, 1, 5, 7), _arith, **GATHER)
  case('sphere_gather', [], b_sphere, ('ERP', 16, 32, 2, 4, 6, 2), _arith, **GATHER)
  case('sphere_gather', [], b_sphere, ('Cassini', 32, 16, 2, 4, 4, 1, 2), _arith, **GATHER)
for _arith in ('f32', 'bf16x6'):
  case('sphere_gather', [], b_sphere, ('ERP', 16, 32, 1, 40, 160), _arith, **GATHER)
case('sphere_gather_scatter', [], b_sphere, ('Cassini', 32, 16, 2, 4, 4, 1, 2, 3, 3, 'gnomonic', False, False, True), 'f32', **GATHER)
for _k in ((1, 3), (2, 2), (5, 5)):
  case('sphere_taps', [], b_sphere, ('ERP', 16, 32, 2, 6, 10, 1, 1) + _k, 'bf16x6', SPHERE_FWD_MIN_WG=0)
case('sphere_random_table', [], b_sphere, ('-', 24, 20, 1, 6, 8, 1, 1, 3, 3, 'random'), 'bf16x6', SPHERE_FWD_MIN_WG=0)

WIN = dict(SPHERE_FWD='window', SPHERE_BWD_WEIGHT='window', SPHERE_FWD_MIN_WG=0, SPHERE_BWD_SPLIT_MIN_WG=0)
for _a in ((33, 66, 1, 12, 40, 1, 2), (10, 20, 2, 5, 7), (36, 72, 1, 8, 12, 1, 2), (32, 64, 3, 40, 16)):
  for _arith in ('f32', 'bf16x6'):
    case('sphere_window', [], b_sphere, ('Cassini',) + _a, _arith, **WIN)
case('sphere_window_nopolar', [], b_sphere, ('Cassini', 33, 66, 1, 12, 40, 1, 2), 'bf16x6', SPHERE_POLAR=False, **WIN)
case('sphere_window_nchw', [], b_sphere, ('Cassini', 36, 72, 1, 8, 12, 1, 2), 'f32', SPHERE_LAYOUT='nchw', **WIN)
# the split and fp16 entries: 16 channels per MFMA on both sides; the adjoint plan needs H % 64 == 0 and W % 4 == 0 of the table
# (Cassini ih = 32, iw = 64: table 64 x 32), the smallest such grid
for _f16 in (True, False):
  case('sphere_window_split', [], b_sphere, ('Cassini', 32, 64, 2, 16, 32, 1, 1, 3, 3, 'gnomonic', _f16, True), 'bf16x6',
       SPHERE_FWD_F16=_f16, SPHERE_BWD_F16=_f16, **WIN)
case('sphere_window_split', [], b_sphere, ('Cassini', 32, 64, 2, 32, 32, 1, 2, 3, 3, 'gnomonic', True, True), 'bf16x6', **WIN)
case('sphere_window_nosplit', [], b_sphere, ('Cassini', 32, 64, 2, 16, 32, 1, 1, 3, 3, 'gnomonic', False, True), 'bf16x6',
     SPHERE_BWD_WEIGHT_SPLIT=False, SPHERE_BWD_DATA_SPLIT=False, **WIN)
for _arith in ('f32', 'bf16x6'):  # an ERP table runs as the Cassini problem of its transposed table, on the NCHW tensors themselves
  case('sphere_window_erp', [], b_sphere, ('ERP', 33, 66, 1, 12, 40, 1, 2), _arith, **WIN)
case('sphere_window_bf16', [], b_sphere, ('Cassini', 33, 66, 1, 12, 40, 1, 2), 'bf16x6', SPHERE_BWD_F16=False, SPHERE_FWD_F16=False, **WIN)
for _arith in ('f32', 'bf16x6'):  # all three window classes and the polar tiles only appear at 128 x 256
  case('sphere_window_128x256', [], b_sphere, ('Cassini', 128, 256, 1, 48, 32, 1, 2, 3, 3, 'gnomonic', True, True), _arith, **WIN)
case('sphere_window_128x256', [], b_sphere, ('Cassini', 128, 256, 1, 48, 32, 1, 2, 3, 3, 'gnomonic', True, True), 'bf16x6', SPHERE_POLAR=False, **WIN)


# ============================================================================================================ 3-D convolutions
@functools.lru_cache(maxsize=None)
def _conv3d_reference(B, Ci, Co, D, H, W, stride, transposed):
  x = _rand((B, Ci, D, H, W), 41)
  if transposed:
    w = _rand((Ci, Co, 3, 3, 3), 48, 0.1)
  else:
    w = _rand((Co, Ci, 3, 3, 3), 42, (2.0 / (27 * Co))**0.5) if Co > 1 else _rand((1, Ci, 3, 3, 3), 55, 0.05)
  xa, wa = x.double().requires_grad_(True), w.double().requires_grad_(True)
  y = F.conv_transpose3d(xa, wa, None, 2, 1, 1) if transposed else F.conv3d(xa, wa, None, stride, 1)
  gy = _rand(tuple(y.shape), 43)
  y.backward(gy.double())
  return x, w, gy, y.detach(), xa.grad, wa.grad


def b_conv3d(B, Ci, Co, D, H, W, stride=1, transposed=False, what='all'):
  """HF.conv3d / HF.deconv3d forward and both gradients (autograd), the weight gradient `into=` a buffer, the input gradient with `acc=`."""
  x, w, gy, y_ref, gx_ref, gw_ref = _conv3d_reference(B, Ci, Co, D, H, W, stride, transposed)
  acc = _rand(tuple(x.shape), 403)

  def run():
    out = {}
    xd, wd, gyd = P(x).requires_grad_(True), P(w).requires_grad_(True), P(gy)
    if what == 'all':
      y = HF.deconv3d(xd, wd) if transposed else HF.conv3d(xd, wd, stride)
      y.backward(gyd)
      out.update(y=y.detach(), gx=xd.grad, gw=wd.grad)
    if what == 'wgrad':
      out['gw'] = HF.conv3d_bwd_weight(gyd, xd.detach(), stride)
      into = PO(torch.ones(w.shape))
      HF.conv3d_bwd_weight(gyd, xd.detach(), stride, into=into)
      out['gw_into'] = into
    if what == 'acc':
      out['gx_acc'] = HF.conv3d_bwd_data(gyd, wd.detach(), tuple(x.shape), stride, acc=P(acc))
      out['gx_plain'] = HF.conv3d_bwd_data(gyd, wd.detach(), tuple(x.shape), stride)
    return out

  def verify(out):
    if 'y' in out:
      if Co == 1 and not transposed:  # test_conv3d_single_output_channel
        close(out, 'y', y_ref, 1e-4, scale=False)
        close(out, 'gx', gx_ref, 1e-4, scale=False)
      else:  # test_conv3d_fwd_bwd, test_conv3d_stride2, test_deconv3d
        close(out, 'y', y_ref, 2e-6 * Ci * 27)
        close(out, 'gx', gx_ref, 2e-6 * Co * 27)
    if 'gw' in out:
      close(out, 'gw', gw_ref, 2e-5)
    if 'gw_into' in out:
      close(out, 'gw_into', gw_ref + 1.0, 2e-5)
    if 'gx_acc' in out:  # test_conv3d_input_gradient_with_a_gradient_already_there: bit for bit what a separate add gives
      assert torch.equal(out['gx_acc'], out['gx_plain'] + acc)
      close(out, 'gx_plain', gx_ref, 2e-6 * Co * 27)

  return run, verify


ARITH3 = [('f32', {}), ('bf16x6', {}), ('bf16x6', {'CONV3D_S1_F16': False})]
for _arith, _sw in ARITH3:
  for _a in ((2, 16, 20, 5, 7, 33), (1, 32, 32, 3, 17, 130), (2, 8, 8, 8, 8, 8)):
    case('conv3d_s1', [], b_conv3d, _a, _arith, **_sw)
  for _a in ((2, 20, 40, 5, 7, 33), (1, 16, 16, 1, 2, 31)):
    case('conv3d_s1_wgrad', [], b_conv3d, _a + (1, False, 'wgrad'), _arith, **_sw)
  for _ci, _co, _v in ((64, 64, (1, 4, 9, 33)), (24, 40, (1, 4, 6, 34))):
    case('conv3d_s1_acc', [], b_conv3d, (_v[0], _ci, _co) + _v[1:] + (1, False, 'acc'), _arith, **_sw)
  for _a in ((1, 20, 1, 3, 5, 33), (2, 32, 1, 1, 1, 7)):
    case('conv3d_head', [], b_conv3d, _a, _arith, **_sw)
for _arith in ('f32', 'bf16x6'):
  for _a in ((2, 20, 40, 4, 6, 70), (1, 32, 64, 4, 8, 64)):
    case('conv3d_s2', [], b_conv3d, _a + (2,), _arith)
  for _a in ((1, 64, 64, 6, 8, 24), (3, 64, 128, 2, 4, 8)):
    case('conv3d_s2_wgrad', [], b_conv3d, _a + (2, False, 'wgrad'), _arith)
  for _ci, _co, _v in ((64, 64, (1, 4, 8, 34)), (40, 24, (1, 4, 6, 34))):
    case('conv3d_s2_acc', [], b_conv3d, (_v[0], _ci, _co) + _v[1:] + (2, False, 'acc'), _arith)
  for _a in ((2, 24, 40, 2, 5, 35), (1, 64, 32, 6, 16, 32), (2, 12, 40, 3, 5, 34), (2, 20, 8, 3, 5, 34)):
    case('deconv3d', [], b_conv3d, _a + (2, True), _arith)


def b_conv3d_bn_eval(Ci, Co, stride, transposed):
  """conv3d_bn_eval / deconv3d_bn_eval in all four relu / add variants: test_folded_batchnorm_conv3d (its shapes 2 x . x 6 x 10 x 36
  and 2 x . x 3 x 5 x 34)."""
  x = _rand((2, Ci, 3, 5, 34), 95) if transposed else _rand((2, Ci, 6, 10, 36), 91)
  w = _rand((Ci, Co, 3, 3, 3), 96, 0.1) if transposed else _rand((Co, Ci, 3, 3, 3), 92, 0.1)
  want = F.conv_transpose3d(x.double(), w.double(), None, 2, 1, 1) if transposed else F.conv3d(x.double(), w.double(), None, stride, 1)
  add = _rand(tuple(want.shape), 94)

  def run():
    out = {}
    with torch.no_grad():
      for relu, with_add in FOLD_VARIANTS:
        bn = _bn_eval_module(Co, 93)
        a = P(add) if with_add else None
        out['y%d%d' % (relu, with_add)] = (HF.deconv3d_bn_eval(P(x), P(w), bn, a, relu) if transposed else
                                           HF.conv3d_bn_eval(P(x), P(w), bn, stride, a, relu))
        if transposed:  # mode_deconv3d_fwd_split_bn (where the split kernel takes the layer) against its _amax twin
          with PlainTwins():
            out['plain%d%d' % (relu, with_add)] = HF.deconv3d_bn_eval(P(x), P(w), _bn_eval_module(Co, 93), a, relu)
    return out

  def verify(out):
    for relu, with_add in FOLD_VARIANTS:
      close(out, 'y%d%d' % (relu, with_add), _unfused(Co, 93, want, add if with_add else None, relu), 1e-4, scale=False)
      if transposed:
        assert torch.equal(out['plain%d%d' % (relu, with_add)], out['y%d%d' % (relu, with_add)]), 'the plain entry equals its _amax twin bit for bit'

  return run, verify


ARITH_EVAL = [('f32', {}), ('bf16x6', {}), ('bf16x6', {'CONV3D_EVAL_F16': False})]
for _arith, _sw in ARITH_EVAL:
  case('conv3d_bn_eval', [], b_conv3d_bn_eval, (20, 40, 1, False), _arith, **_sw)
  case('conv3d_bn_eval', [], b_conv3d_bn_eval, (64, 64, 1, False), _arith, **_sw)
  case('conv3d_bn_eval', [], b_conv3d_bn_eval, (32, 64, 2, False), _arith, **_sw)
  case('deconv3d_bn_eval', [], b_conv3d_bn_eval, (64, 32, 2, True), _arith, **_sw)
for _arith in ('f32', 'bf16x6'):
  case('conv3d_bn_eval', [], b_conv3d_bn_eval, (16, 24, 2, False), _arith)
  for _ci, _co in ((12, 40), (24, 40), (20, 8)):
    case('deconv3d_bn_eval', [], b_conv3d_bn_eval, (_ci, _co, 2, True), _arith)


def b_conv3d_stats(B, Ci, Co, D, H, W, relu, with_add):
  """test_conv3d_with_batchnorm_statistics_in_its_epilogue: mode_conv3d_fwd_split_stats + mode_bn_train_fwd_prestats(_amax)."""
  x = _rand((B, Ci, D, H, W), 301) + 3.0
  w = _rand((Co, Ci, 3, 3, 3), 302, (2.0 / (27 * Ci))**0.5) + 0.02
  add = _rand((B, Co, D, H, W), 303) if with_add else None
  gout = _rand((B, Co, D, H, W), 304)

  def once():
    bn = nn.BatchNorm3d(Co).to(DEV)
    for name in ('weight', 'bias', 'running_mean', 'running_var'):
      getattr(bn, name).data = P(getattr(bn, name).data.cpu())
    xd, wd = P(x).requires_grad_(True), P(w).requires_grad_(True)
    assert HF.conv3d_stats_supported(xd, wd, bn)
    o = HF.conv3d_bn_train(xd, wd, bn, P(add) if with_add else None, relu)
    o.backward(P(gout))
    return {'out': o.detach(), 'gx': xd.grad, 'gw': wd.grad, 'ggamma': bn.weight.grad, 'rm': bn.running_mean.detach(), 'rv': bn.running_var.detach()}

  def run():
    out = once()
    with PlainTwins():
      plain = once()
    out.update({'plain_' + k: v for k, v in plain.items()})
    return out

  def verify(out):
    conv64, bn64 = nn.Conv3d(Ci, Co, 3, 1, 1, bias=False).double(), nn.BatchNorm3d(Co).double()
    with torch.no_grad():
      conv64.weight.copy_(w.double())
    xa = x.double().requires_grad_(True)
    o = bn64(conv64(xa))
    o = o + add.double() if with_add else o
    o = torch.relu(o) if relu else o
    o.backward(gout.double())
    close(out, 'out', o.detach(), 2e-4)
    close(out, 'gx', xa.grad, 2e-4)
    close(out, 'gw', conv64.weight.grad, 2e-4)
    close(out, 'ggamma', bn64.weight.grad, 2e-4)
    close(out, 'rm', 0.1 * conv64(x.double()).transpose(0, 1).reshape(Co, -1).mean(1).detach(), 1e-4)
    close(out, 'rv', bn64.running_var, 1e-3)
    for k in ('out', 'gx', 'gw', 'ggamma', 'rm', 'rv'):
      assert torch.equal(out[k], out['plain_' + k]), 'mode_bn_train_fwd_prestats equals its _amax twin bit for bit (%s)' % k

  return run, verify


for _relu, _with_add in ((True, False), (False, True)):
  case('conv3d_stats', ['mode_conv3d_fwd_split_stats', 'mode_bn_train_fwd_prestats', 'mode_bn_train_fwd_prestats_amax'], b_conv3d_stats,
       (1, 32, 64, 5, 9, 33, _relu, _with_add), 'bf16x6', CONV3D_BN_STATS=True)


# ============================================================================================================ 2-D convolutions
def b_conv2d(B, Ci, Co, H, W, dil):
  """The 3 x 3 stride-1 layers: test_conv2d_3x3_kernels (forward, input gradient, `acc=`, weight gradient, `into=`), eval fold."""
  x, w = _rand((B, Ci, H, W), 61), _rand((Co, Ci, 3, 3), 62, 0.2)
  xa, wa = x.double().requires_grad_(True), w.double().requires_grad_(True)
  y_ref = F.conv2d(xa, wa, None, 1, dil, dil)
  gy = _rand(tuple(y_ref.shape), 63)
  y_ref.backward(gy.double())
  y_ref, acc, add = y_ref.detach(), _rand(tuple(x.shape), 413), _rand(tuple(y_ref.shape), 102)

  def run():
    xd, wd, gyd = P(x), P(w), P(gy)
    out = {'gw': HF.conv2d_bwd_weight(gyd, xd, dil)}
    into = PO(torch.ones(w.shape))
    HF.conv2d_bwd_weight(gyd, xd, dil, into=into)
    out['gw_into'] = into
    for f16 in (False, True):
      out['y%d' % f16] = HF.conv2d_fwd(xd, wd, dil, f16=f16)
      out['gx%d' % f16] = HF.conv2d_bwd_data(gyd, wd, dil, f16=f16)
      out['gx_acc%d' % f16] = HF.conv2d_bwd_data(gyd, wd, dil, acc=P(acc), f16=f16)
    xg, wg = P(x).requires_grad_(True), P(w).requires_grad_(True)
    y = HF.conv2d_3x3(xg, wg, dil)
    y.backward(gyd)
    out.update(fn_y=y.detach(), fn_gx=xg.grad, fn_gw=wg.grad)
    with torch.no_grad():
      for relu, with_add in ((True, True), (False, False)):
        out['bn%d%d' % (relu, with_add)] = HF.conv2d_bn_eval(xd, wd, _bn_eval_module(Co, 101, 2), dil, P(add) if with_add else None, relu)
    return out

  def verify(out):
    close(out, 'gw', wa.grad, 2e-5)
    close(out, 'gw_into', wa.grad + 1.0, 2e-5)
    close(out, 'fn_gw', wa.grad, 2e-5)
    for f16 in (0, 1):
      close(out, 'y%d' % f16, y_ref, 2e-6 * (Ci * 9))
      close(out, 'gx%d' % f16, xa.grad, 2e-6 * (Co * 9))
      assert torch.equal(out['gx_acc%d' % f16], out['gx%d' % f16] + acc)  # test_conv3d_input_gradient_with_a_gradient_already_there
    close(out, 'fn_y', y_ref, 2e-6 * (Ci * 9))
    close(out, 'fn_gx', xa.grad, 2e-6 * (Co * 9))
    for relu, with_add in ((True, True), (False, False)):  # test_folded_batchnorm_conv2d_3x3
      close(out, 'bn%d%d' % (relu, with_add), _unfused(Co, 101, y_ref, add if with_add else None, relu), 1e-4, scale=False)

  return run, verify


ARITH2 = [('f32', {}), ('bf16x6', {}), ('bf16x6', {'CONV2D_F16': False, 'CONV2D_EVAL_F16': False})]
for _arith, _sw in ARITH2:
  for _a in ((2, 20, 40, 7, 33, 1), (1, 8, 8, 3, 5, 2), (1, 16, 40, 9, 31, 2), (1, 32, 64, 9, 33, 2)):
    case('conv2d_3x3', [], b_conv2d, _a, _arith, **_sw)


def b_conv2d_layers(B, Ci, Co, H, W, k, s, p, need_gx=True):
  """The other nn.Conv2d layers through models.stage3d (conv3 in training, conv_bn in eval): 1 x 1 GEMMs, the 7 x 7 stem, the stride-2
  3 x 3 layer (mode_zero_insert2 + the stride-1 kernels), integer-table kernels.  test_conv1x1_kernels, test_conv_stem_kernels,
  test_conv2d_3x3_stride2_layer, test_conv2d_on_the_integer_table, test_folded_batchnorm_other_conv2d_layers."""
  from models import stage3d
  x = _rand((B, Ci, H, W), 122)
  w = _rand((Co, Ci, k, k), 121, (2.0 / (Ci * k * k))**0.5)
  xa, wa = x.double().requires_grad_(True), w.double().requires_grad_(True)
  y_ref = F.conv2d(xa, wa, None, s, p)
  gy = _rand(tuple(y_ref.shape), 123)
  y_ref.backward(gy.double())
  y_ref, add = y_ref.detach(), _rand(tuple(y_ref.shape), 125)

  def run():
    _fresh_caches()
    conv = nn.Conv2d(Ci, Co, k, s, p, bias=False).to(DEV)
    conv.weight.data = P(w)
    xd = P(x).requires_grad_(need_gx)
    y = stage3d.conv3(conv, xd)
    y.backward(P(gy))
    out = {'y': y.detach(), 'gw': conv.weight.grad}
    if need_gx:
      out['gx'] = xd.grad
    with torch.no_grad():
      for relu, with_add in ((True, True), (False, False)):
        seq = nn.Sequential(conv, _bn_eval_module(Co, 124, 2)).eval()
        out['bn%d%d' % (relu, with_add)] = stage3d.conv_bn(seq, P(x), relu, P(add) if with_add else None)
    return out

  def verify(out):
    close(out, 'y', y_ref, 2e-6 * Ci * k * k)
    if need_gx:
      close(out, 'gx', xa.grad, 2e-6 * Co * k * k)
    close(out, 'gw', wa.grad, 2e-5)
    for relu, with_add in ((True, True), (False, False)):
      close(out, 'bn%d%d' % (relu, with_add), _unfused(Co, 124, y_ref, add if with_add else None, relu), 1e-4, scale=False)

  return run, verify


for _a in ((1, 5, 7, 3, 12, 1, 1, 0), (2, 12, 200, 6, 8, 1, 1, 0), (1, 10, 6, 6, 16, 1, 2, 0), (2, 16, 24, 7, 16, 1, 2, 0), (2, 8, 8, 16, 24, 1, 2, 0)):
  case('conv1x1', [], b_conv2d_layers, _a, 'bf16x6')
for _a in ((2, 3, 20, 26, 70, 7, 2, 3, False), (1, 3, 32, 8, 8, 7, 2, 3, False)):
  case('conv_stem', [], b_conv2d_layers, _a, 'bf16x6')
for _arith in ('f32', 'bf16x6'):
  for _a in ((2, 8, 8, 2, 4, 3, 2, 1), (1, 20, 40, 10, 36, 3, 2, 1)):
    case('conv2d_3x3_s2', [], b_conv2d_layers, _a, _arith)
case('conv2d_tabled', [], b_conv2d_layers, (1, 5, 7, 9, 11, 3, 2, 1), 'bf16x6')
case('conv2d_tabled', [], b_conv2d_layers, (1, 6, 4, 10, 13, 5, 3, 2), 'bf16x6')


# ============================================================================================================ BatchNorm, classifier head
def b_bn_act(shape, relu, with_add, groups=1):
  """test_bn_act_train_and_eval / test_bn_act_grouped_statistics, and the plain entries against their `_amax` twins."""
  C = shape[1]
  BN = nn.BatchNorm3d if len(shape) == 5 else nn.BatchNorm2d
  gen = torch.Generator().manual_seed(7)
  gamma, beta = 1 + 0.2 * torch.randn(C, generator=gen), 0.3 * torch.randn(C, generator=gen)
  y = _rand(shape, 71, 2.0) + 1.5 + torch.arange(shape[0]).view(-1, *([1] * (len(shape) - 1))).float() * (groups > 1)
  add = _rand(shape, 72) if with_add else None
  gout = _rand(shape, 73)

  def once():
    bn = BN(C).to(DEV)
    bn.weight.data, bn.bias.data = P(gamma), P(beta)
    bn.running_mean.data, bn.running_var.data = P(torch.zeros(C)), P(torch.ones(C))
    yd = P(y).requires_grad_(True)
    ad = P(add).requires_grad_(True) if with_add else None
    o = HF.bn_act(bn, yd, ad, relu, groups=groups)
    o.backward(P(gout))
    res = {'out': o.detach(), 'gy': yd.grad, 'ggamma': bn.weight.grad, 'gbeta': bn.bias.grad, 'rm': bn.running_mean.detach().clone(),
           'rv': bn.running_var.detach().clone()}
    if with_add:
      res['gadd'] = ad.grad
    bn.eval()
    with torch.no_grad():
      res['eval'] = HF.bn_act(bn, P(y), P(add) if with_add else None, relu)
    return res

  def run():
    out = once()
    with PlainTwins():
      plain = once()
    out.update({'plain_' + k: v for k, v in plain.items()})
    return out

  def verify(out):
    ref_bn = BN(C).double()
    with torch.no_grad():
      ref_bn.weight.copy_(gamma)
      ref_bn.bias.copy_(beta)
    ya = y.double().requires_grad_(True)
    aa = add.double().requires_grad_(True) if with_add else None
    outs, pre = [], []
    for part, apart in zip(ya.chunk(groups, 0), aa.chunk(groups, 0) if with_add else [None] * groups):
      o = ref_bn(part)
      o = o + apart if with_add else o
      pre.append(o.detach())
      outs.append(torch.relu(o) if relu else o)
    o_ref = torch.cat(outs, 0)
    o_ref.backward(gout.double())
    assert int((torch.cat(pre, 0).abs() < 1e-5).sum()) == 0 or not relu, 'an element within fp32 round-off of the ReLU threshold: pick another seed'
    close(out, 'out', o_ref.detach(), 2e-5, scale=False)
    close(out, 'gy', ya.grad, 5e-5)
    if with_add:
      close(out, 'gadd', aa.grad, 1e-6, scale=False)
    close(out, 'ggamma', ref_bn.weight.grad, 1e-4)
    close(out, 'gbeta', ref_bn.bias.grad, 1e-4)
    close(out, 'rm', ref_bn.running_mean, 1e-5, scale=False)
    close(out, 'rv', ref_bn.running_var, 1e-4, scale=False)
    ref_bn.eval()
    with torch.no_grad():
      e = ref_bn(y.double())
      e = e + add.double() if with_add else e
      e = torch.relu(e) if relu else e
    close(out, 'eval', e, 2e-5, scale=False)
    for k in [k for k in out if not k.startswith('plain_')]:
      assert torch.equal(out[k], out['plain_' + k]), 'mode_bn_train_fwd / _bwd equal their _amax twins bit for bit (%s)' % k

  return run, verify


BN_ENTRIES = ['mode_bn_train_fwd', 'mode_bn_train_bwd', 'mode_bn_train_fwd_amax', 'mode_bn_train_bwd_amax', 'mode_bn_eval_fwd']
for _relu, _with_add in FOLD_VARIANTS:
  for _shape in ((3, 5, 2, 2, 4), (2, 6, 3, 5, 7), (2, 16, 9, 11)):
    case('bn_act', BN_ENTRIES, b_bn_act, (_shape, _relu, _with_add), 'bf16x6')
  case('bn_act_groups', BN_ENTRIES, b_bn_act, ((4, 6, 7, 9), _relu, _with_add, 2), 'bf16x6')
case('bn_act', BN_ENTRIES, b_bn_act, ((2, 6, 3, 5, 7), True, True), 'f32')


@functools.lru_cache(maxsize=None)
def _classif_reference(B, C, vol, with_add):
  """Inputs and the float64 reference of one classifier case, computed once and shared by its two arithmetics (nothing writes to them)."""
  import test_gpu_classif as TC
  D, H, W = vol
  y = _rand((B, C, D, H, W), 1) * 1.7 + 0.4
  add = _rand((B, 1, D, H, W), 2) if with_add else None
  go = _rand((B, 1, D, H, W), 3)
  bn, conv = TC._modules(C, 10)
  return y, add, go, TC._reference(y, add, go, bn, conv)


def b_classif(B, C, vol, with_add, off_grid=False, clear_of_the_threshold=False):
  """test_gpu_classif.test_fused_classifier_head_small_and_ragged.
  off_grid: the BACKWARD reads y from a contiguous view one element into a larger buffer (4 bytes off the 16-byte grid:
  mode_classif_train_bwd must take its dword kernels although W % 4 == 0); the elements around the view are NaN, so a 16-byte access
  over its ends shows.  The forward runs on an aligned copy: its statistics pass reads rows that are multiples of 16 bytes in 16-byte
  pieces and refuses such a view ("mode_classif_train_fwd: unaligned buffer"), so the view reaches the backward's own host code
  (ClassifHeadFunction.backward) through a stand-in for the autograd context that holds the forward's saved tensors.
  clear_of_the_threshold: the case was chosen to have NO element within 1e-5 of the ReLU threshold in float64 -- every element of gy is
  compared, none is left out."""
  import test_gpu_classif as TC
  D, H, W = vol
  y, add, go, want = _classif_reference(B, C, tuple(vol), with_add)

  def once():
    bn, conv = TC._modules(C, 10)
    bn, conv = bn.to(DEV), conv.to(DEV)
    for m, names in ((bn, ('weight', 'bias', 'running_mean', 'running_var', 'num_batches_tracked')), (conv, ('weight',))):
      for name in names:
        getattr(m, name).data = P(getattr(m, name).data.cpu())
    yd = P(y).requires_grad_(True)
    assert yd.data_ptr() % 16 == 0
    ad = P(add).requires_grad_(True) if with_add else None
    assert HF.classif_fused_supported(yd, bn, conv)
    cost = HF.classif_head_train(yd, bn, conv, ad)
    out = {'cost': cost.detach(), 'rm': bn.running_mean.detach(), 'rv': bn.running_var.detach(), 'nbt': bn.num_batches_tracked.detach()}
    if off_grid:
      buf = torch.full((y.numel() + 4,), float('nan'))
      buf[1:1 + y.numel()] = y.reshape(-1)
      y_off = PO(buf)[1:1 + y.numel()].view(y.shape)
      assert y_off.is_contiguous() and y_off.data_ptr() % 16 == 4 and W % 4 == 0

      class Ctx(object):  # what ClassifHeadFunction.backward reads of its context
        saved_tensors = (y_off,) + tuple(cost.grad_fn.saved_tensors[1:])
        needs_input_grad = (True, True, True, True, with_add) + (False,) * 5
        has_add = with_add

      grads = HF.ClassifHeadFunction.backward(Ctx, P(go))
      out.update(zip(('gy', 'gw', 'ggamma', 'gbeta'), grads[:4]))
      if with_add:
        out['gadd'] = grads[4]
      return out
    cost.backward(P(go))
    out.update({'gy': yd.grad, 'gw': conv.weight.grad, 'ggamma': bn.weight.grad, 'gbeta': bn.bias.grad})
    if with_add:
      out['gadd'] = ad.grad
    return out

  def run():
    out = once()
    with PlainTwins():  # mode_classif_train_bwd against its _amax twin
      out.update({'plain_' + k: v for k, v in once().items()})
    return out

  def verify(out):
    n = B * D * H * W
    TC._check('cost', out['cost'], want[0], 2.0**-22 * np.sqrt(27 * C) * 8)
    if clear_of_the_threshold:
      n_near = int((want[8].abs() <= 1e-5).sum())
      assert n_near == 0, n_near
    TC._check_off_the_relu_threshold('gy', out['gy'], want[1], want[8], 2e-5)
    if with_add:
      TC._check('gadd', out['gadd'], want[2], 1e-6)
    TC._check('gw', out['gw'], want[3], 2.0**-22 * np.sqrt(n) * 8)
    TC._check('ggamma', out['ggamma'], want[4], 2.0**-22 * np.sqrt(n * 27) * 8)
    TC._check('gbeta', out['gbeta'], want[5], 2.0**-22 * np.sqrt(n * 27) * 8)
    TC._check('running_mean', out['rm'], want[6], 1e-6)
    TC._check('running_var', out['rv'], want[7], 1e-5)
    assert int(out['nbt']) == 1
    for k in [k for k in out if not k.startswith('plain_')]:
      assert torch.equal(out[k], out['plain_' + k]), 'mode_classif_train_bwd equals its _amax twin bit for bit (%s)' % k

  return run, verify


for _arith in ('f32', 'bf16x6'):
  for _a in ((2, 5, (5, 11, 37), True), (1, 32, (13, 20, 70), True)):
    case('classif_head', [], b_classif, _a, _arith)


# ============================================================================================================ soft-argmin head
@functools.lru_cache(maxsize=None)
def _head_reference(B, D4, H4, W4, size, border):
  """Logits, the two upstream gradients (the confidence's zeroed where the float64 prediction lies within 1e-3 of a half-integer, and
  the share of such pixels) and the float64 reference (conf_grad_ref.head_reference: oracle/mode_ref.py under autograd) of one head case,
  computed once and shared (nothing writes to them).  border: +14 on node 0 over the first W4 // 3 columns and on node D4 - 1 over the
  last W4 // 3 -- predictions that round to 0 and to D - 1, where a window index counts twice and the confidence exceeds 1."""
  import conf_grad_ref as C
  lg = _rand((B, 1, D4, H4, W4), 61, 3.0)
  if border:
    lg[:, :, 0, :, :W4 // 3] += 14.0
    lg[:, :, D4 - 1, :, W4 - W4 // 3:] += 14.0
  gp = _rand((B, 1) + size[1:], 62)
  gc, zeroed = C.masked_gconf(lg, _rand((B, 1) + size[1:], 63), size)
  return lg, gp, gc, zeroed, C.head_reference(lg, gp, gc, size)


def b_head(B, D4, H4, W4, scale_or_size, conf_grad=False, border=False, loss_supported=None):
  """test_head_fwd_bwd_conf (bounds 1e-4 D, 1e-4 x max|g|, 1e-4 on the stable confidences; at most 1 % of the pixels may be unstable).
  conf_grad: also mode_head_bwd_conf as test_head_bwd_conf_against_float64 has it (both terms, the confidence term alone, and the bits
  of mode_head_bwd without a confidence gradient).  loss_supported: what HF.head_loss_supported must say of the shape, i.e. which form
  the backward's routing takes.  border: the logits of _head_reference that put confidence windows at both ends of the disparity axis."""
  D, H, W = size = tuple(scale_or_size) if isinstance(scale_or_size, tuple) else (D4 * scale_or_size, H4 * scale_or_size, W4 * scale_or_size)
  lg, g, gc, zeroed, ref = _head_reference(B, D4, H4, W4, size, border)
  bits = lambda t: t.view(torch.int32)

  def run():
    ld = P(lg).requires_grad_(True)
    if loss_supported is not None:
      assert bool(HF.head_loss_supported(ld, size)) == loss_supported, 'the routing of this shape changed: it no longer reaches the form it is here for'
    pred = HF.head(ld, size)
    pred.backward(P(g))
    p2, conf = HF.head_fwd(P(lg), size, with_confidence=True)
    out = {'pred': pred.detach(), 'gl': ld.grad, 'pred2': p2, 'conf': conf}
    if conf_grad:
      logits, gp, gcd = P(lg), P(g), P(gc)
      out['gl_both'] = HF.head_bwd_conf(logits, p2, conf, gp, gcd, size)
      out['gl_conf'] = HF.head_bwd_conf(logits, p2, conf, P(torch.zeros_like(g)), gcd, size)
      out['gl_no_gconf'] = HF.head_bwd_conf(logits, p2, conf, gp, P(torch.zeros_like(gc)), size)
      out['gl_plain'] = HF.head_bwd(logits, gp, size)
    return out

  def verify(out):
    close(out, 'pred', ref['pred'], 1e-4 * D, scale=False)
    close(out, 'gl', ref['g_pred'], 1e-4)
    assert torch.equal(out['pred2'], out['pred'])
    print('  %.3f %% of the pixels within 1e-3 of a half-integer (confidence left out, gconf zeroed)' % (100 * zeroed))
    assert zeroed <= 0.01
    err = float((out['conf'].double() - ref['conf']).abs()[~ref['unstable']].max())
    print('  conf: max err %.3e (bound %.3e)' % (err, 1e-4))
    assert err < 1e-4
    if border:
      r = ref['pred'].round()
      low, high, top = float((r == 0).double().mean()), float((r == D - 1).double().mean()), float(ref['conf'].max())
      print('  %.1f %% of the predictions round to 0, %.1f %% to D - 1; largest confidence %.3f' % (100 * low, 100 * high, top))
      assert low >= 0.05 and high >= 0.05 and top > 1.5
    if conf_grad:
      close(out, 'gl_both', ref['g_pred'] + ref['g_conf'], 1e-4)
      close(out, 'gl_conf', ref['g_conf'], 1e-4)
      assert float(ref['g_conf'].abs().max()) > 0
      differ = int((bits(out['gl_no_gconf']) != bits(out['gl_plain'])).sum())
      assert differ == 0, 'mode_head_bwd_conf with gconf == 0 has the bits of mode_head_bwd (include/mode_hip.h): %d elements differ' % differ
      assert torch.equal(bits(out['gl_plain']), bits(out['gl']))  # (HF.head's backward IS head_bwd)

  return run, verify


case('head', ['mode_head_fwd', 'mode_head_bwd'], b_head, (1, 12, 5, 7, 4))
case('head', ['mode_head_fwd', 'mode_head_bwd'], b_head, (1, 3, 4, 4, 3))
case('head_two_kernel_bwd', ['mode_head_fwd', 'mode_head_bwd'], b_head, (1, 4, 2, 100, (16, 8, 512)))


def b_head_loss(B, D4, H4, W4):
  """The inputs of test_head_loss_fused_equals_the_torch_composition, against float64 (that test compares two fp32 evaluations): the
  predictions and the logits' gradients under the bounds of test_head_fwd_bwd_conf (1e-4 D; 1e-4 of the largest gradient); the loss
  within 2.2e-4 D -- smooth-L1 is 1-Lipschitz, so the weighted mean (0.5 + 0.7 + 1.0) moves by at most 2.2 x the predictions' bound."""
  from oracle import mode_ref
  D, H, W = 4 * D4, 4 * H4, 4 * W4
  costs = [_rand((B, 1, D4, H4, W4), 70 + i) * 2 for i in range(3)]
  gt = torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(5)) * (D / 2)
  gt[torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(6)) < 0.1] = float('nan')
  gt[0, 0, :2, :5] = 3 * D

  def run():
    cs = [P(c).requires_grad_(True) for c in costs]
    gd = GB.place(gt.to(DEV), is_input=False)  # (NaN marks the pixels without ground truth: outputs must be finite all the same)
    assert HF.head_loss_supported(cs[0], (D, H, W))
    count = (~torch.isnan(gd)).sum().float()
    loss, preds = HF.head_loss(cs, (D, H, W), gd, count.reciprocal())
    loss.backward()
    return {'loss': loss.detach(), 'preds': list(preds), 'grads': [c.grad for c in cs]}

  def verify(out):
    mask = ~torch.isnan(gt)
    ca = [c.double().requires_grad_(True) for c in costs]
    ref = 0
    for i, (wgt, c) in enumerate(zip((0.5, 0.7, 1.0), ca)):
      o = mode_ref.disparity_head(c, D, H, W)
      close(out, 'preds[%d]' % i, o.detach(), 1e-4 * D, scale=False)
      ref = ref + wgt * F.smooth_l1_loss(o[mask], gt.double()[mask])
    ref.backward()
    print('  loss: err %.3e (bound %.3e)' % (abs(float(out['loss']) - float(ref)), 2.2e-4 * D))
    assert abs(float(out['loss']) - float(ref)) <= 2.2e-4 * D
    for i, c in enumerate(ca):
      close(out, 'grads[%d]' % i, c.grad, 1e-4 * max(1.0, float(c.grad.abs().max())), scale=False)

  return run, verify


case('head_loss', ['mode_head_fwd', 'mode_smooth_l1_masked', 'mode_head_bwd_loss'], b_head_loss, (2, 4, 16, 8))


# ============================================================================================================ small operators
def b_small(n):
  x = _rand((n,), 5, 3.0)
  xs = [_rand((n,), 6 + i) for i in range(5)]

  def run():
    xd = P(x)
    out = {'amax': HF.abs_max(xd), 'sum2': HF.sum_n([P(t) for t in xs[:2]]), 'sum3': HF.sum_n([P(t) for t in xs[:3]]),
           'sum5': HF.sum_n([P(t) for t in xs])}
    ptrs = P(torch.tensor([xd.data_ptr(), out['sum2'].data_ptr()], dtype=torch.int64))
    counts = P(torch.tensor([n, n], dtype=torch.int64))
    batch = PO(torch.full((2, HF.BN_ABSMAX_FLOATS), float('nan')))
    mode_hip.check(mode_hip.lib().mode_abs_max_batch(mode_hip.ptr(ptrs), mode_hip.ptr(counts), 2, mode_hip.ptr(batch), mode_hip.stream_of(batch)),
                   'mode_abs_max_batch')
    out['amax_batch'] = batch
    return out

  def verify(out):  # test_abs_max_is_exact_and_order_independent: a maximum is exact
    assert float(out['amax'].max()) == float(x.abs().max()) and float(out['amax'].min()) >= 0
    assert float(out['amax_batch'][0].max()) == float(x.abs().max())
    assert float(out['amax_batch'][1].max()) == float(out['sum2'].abs().max())
    # ((a + b) + c) + d in fp32: one rounding of at most 2^-24 of the partial sum per addition; twice that as the bound
    close(out, 'sum2', xs[0].double() + xs[1].double(), 2.0**-23)
    close(out, 'sum3', sum(t.double() for t in xs[:3]), 2 * 2.0**-23)
    close(out, 'sum5', sum(t.double() for t in xs), 4 * 2.0**-23)

  return run, verify


for _n in (1, 1023, 4097):
  case('small_ops', ['mode_abs_max', 'mode_abs_max_batch', 'mode_sum_n'], b_small, (_n,))


def b_planes():
  x = _rand((2, 3, 7, 33), 8)
  gy = _rand((2, 3, 3, 16), 9)

  def run():
    xd = P(x)
    t = HF.transpose_planes(xd)
    back = PO(torch.full(x.shape, float('nan')))
    HF.transpose_planes(t, back)
    up = PO(torch.full((2, 3, 6, 32), float('nan')))
    mode_hip.check(mode_hip.lib().mode_zero_insert2(mode_hip.ptr(P(gy)), mode_hip.ptr(up), 6, 3, 16, None), 'mode_zero_insert2')
    return {'t': t, 'back': back, 'up': up}

  def verify(out):  # exact data movement (test_conv2d_3x3_stride2_layer for the zero insertion)
    assert torch.equal(out['t'], x.transpose(2, 3)) and torch.equal(out['back'], x)
    want = torch.zeros(2, 3, 6, 32)
    want[:, :, ::2, ::2] = gy
    assert torch.equal(out['up'], want)

  return run, verify


case('planes', ['mode_transpose_planes', 'mode_zero_insert2'], b_planes)


# ============================================================================================================ fusion operators
def b_maxpool(shape):
  g = torch.Generator().manual_seed(3)
  x = torch.randn(*shape, generator=g)
  x[0, 0, :2, :2] = 1.5  # a tie
  go = torch.randn(shape[0], shape[1], shape[2] // 2, shape[3] // 2, generator=g)

  def run():
    xd = P(x).requires_grad_(True)
    y = HF.maxpool2x2(xd)
    y.backward(P(go))
    return {'y': y.detach(), 'gx': xd.grad}

  def verify(out):  # test_gpu_maxpool2x2_is_torchs: bit for bit
    xr = x.clone().requires_grad_(True)
    y_ref = F.max_pool2d(xr, 2, 2)
    y_ref.backward(go)
    assert torch.equal(out['y'], y_ref.detach()) and torch.equal(out['gx'], xr.grad)

  return run, verify


for _shape in ((1, 3, 9, 7), (1, 2, 2, 2)):
  case('maxpool2x2', ['mode_maxpool2x2_fwd', 'mode_maxpool2x2_bwd'], b_maxpool, (_shape,))


def b_deconv2x2(B, Ci, Co, H, W):
  """test_gpu_deconv2x2_against_float64."""
  torch.manual_seed(5)
  conv = nn.ConvTranspose2d(Ci, Co, 2, 2)
  x, go = torch.randn(B, Ci, H, W), torch.randn(B, Co, 2 * H, 2 * W)
  sd = {k: v.clone() for k, v in conv.state_dict().items()}
  bnv = {'running_mean': torch.randn(Co), 'running_var': torch.rand(Co) * 1.5 + 0.5, 'weight': torch.rand(Co) + 0.5, 'bias': torch.randn(Co)}

  def run():
    convd = nn.ConvTranspose2d(Ci, Co, 2, 2).to(DEV)
    convd.weight.data, convd.bias.data = P(sd['weight']), P(sd['bias'])
    xd = P(x).requires_grad_(True)
    assert HF.deconv2x2_supported(xd, convd)
    y = HF.deconv2x2(xd, convd)
    y.backward(P(go))
    bn = nn.BatchNorm2d(Co).to(DEV).eval()
    for k, v in bnv.items():
      getattr(bn, k).data = P(v)
    with torch.no_grad():
      ev = HF.deconv2x2_bn_eval(P(x), convd, bn, True)
    return {'y': y.detach(), 'gx': xd.grad, 'gw': convd.weight.grad, 'gb': convd.bias.grad, 'eval': ev}

  def verify(out):
    c64 = nn.ConvTranspose2d(Ci, Co, 2, 2).double()
    c64.load_state_dict({k: v.double() for k, v in sd.items()})
    x64 = x.double().requires_grad_(True)
    y64 = c64(x64)
    y64.backward(go.double())
    tol = 2e-6 * Ci ** 0.5
    close(out, 'y', y64.detach(), tol)
    close(out, 'gx', x64.grad, 4 * tol)
    close(out, 'gw', c64.weight.grad, 2e-6 * (B * H * W) ** 0.5)
    close(out, 'gb', c64.bias.grad, 1e-5)
    bn = nn.BatchNorm2d(Co).double().eval()
    with torch.no_grad():
      for k, v in bnv.items():
        getattr(bn, k).copy_(v)
      close(out, 'eval', torch.relu(bn(y64.detach())), 4 * tol)

  return run, verify


case('deconv2x2', ['mode_depth_to_space2', 'mode_space_to_depth2'], b_deconv2x2, (2, 16, 8, 6, 8))


def b_conv1x1_sigmoid(B, C, H, W):
  """test_gpu_conv1x1_sigmoid_against_float64."""
  torch.manual_seed(6)
  conv = nn.Conv2d(C, 1, 1, bias=True)
  x, go = torch.randn(B, C, H, W), torch.randn(B, 1, H, W)
  sd = {k: v.clone() for k, v in conv.state_dict().items()}

  def run():
    convd = nn.Conv2d(C, 1, 1, bias=True).to(DEV)
    convd.weight.data, convd.bias.data = P(sd['weight']), P(sd['bias'])
    xd = P(x).requires_grad_(True)
    assert HF.conv1x1_sigmoid_supported(xd, convd)
    s_ = HF.conv1x1_sigmoid(xd, convd)
    s_.backward(P(go))
    return {'s': s_.detach(), 'gx': xd.grad, 'gw': convd.weight.grad, 'gb': convd.bias.grad}

  def verify(out):
    c64 = nn.Conv2d(C, 1, 1, bias=True).double()
    c64.load_state_dict({k: v.double() for k, v in sd.items()})
    x64 = x.double().requires_grad_(True)
    s64 = torch.sigmoid(c64(x64))
    s64.backward(go.double())
    close(out, 's', s64.detach(), 2e-6, scale=False)
    close(out, 'gx', x64.grad, 2e-6)
    close(out, 'gw', c64.weight.grad, 1e-5)
    close(out, 'gb', c64.bias.grad, 1e-5)

  return run, verify


case('conv1x1_sigmoid', ['mode_conv1x1_sigmoid_fwd', 'mode_conv1x1_sigmoid_bwd'], b_conv1x1_sigmoid, (1, 8, 6, 10))


# ============================================================================================================ metrics, ERP scoring
def b_metrics(n):
  """masked_metrics and the SILog loss on unaligned slices.  Counts exactly (test_gpu_odd_sizes_and_unaligned_slices); the sum of the
  fp32 terms |p - g| in float64 to n 2^-53 <= 1e-12 relative (any order of a float64 sum of n <= 4097 terms); the loss to 1e-6 of
  max(|loss|, mean l^2) and its gradient to 1e-6 in relative L2 norm (test_gpu_silog_loss_golden_cases, _matches_float64_autograd)."""
  g = torch.Generator().manual_seed(n)
  gt = torch.rand(n + 6, generator=g) * 60
  pred = gt * (1 + 0.3 * torch.randn(n + 6, generator=g))
  gt[::53] = 0
  pred[5::41] = -1
  mask = (torch.arange(n) % 7) != 3

  def run():
    p, gg = P(pred)[1:1 + n], P(gt)[3:3 + n]  # 4- and 12-byte offsets into the guarded buffers
    m = P(torch.cat([torch.zeros(1, dtype=torch.bool), mask]))[1:]  # a mask at an odd byte
    stats = HF.masked_metrics(p, gg, m, px=(1, 3), d1=((3, 0.05),), ratio=(1.25,))
    pr = p.detach().requires_grad_(True)
    loss = HF.silog_loss(pr, gg, m)
    loss.backward()
    return {'stats': torch.from_numpy(stats), 'loss': loss.detach(), 'gp': pr.grad}

  def verify(out):
    pc, gc = pred[1:1 + n][mask], gt[3:3 + n][mask]
    s = out['stats'].numpy()
    e = (pc - gc).abs()
    assert s[mode_hip.M_N] == pc.numel() and s[mode_hip.M_N_GT] == int((gc > 0).sum()) and s[mode_hip.M_N_BOTH] == int(((gc > 0) & (pc > 0)).sum())
    assert s[mode_hip.M_PX] == int((e >= 1).sum()) and s[mode_hip.M_PX + 1] == int((e >= 3).sum())
    assert s[mode_hip.M_RATIO] == int((torch.max(pc / gc, gc / pc) < 1.25).sum())
    assert abs(s[mode_hip.M_SUM_ABS] - float(e.double().sum())) <= 1e-12 * max(1.0, float(e.double().sum()))
    assert s[mode_hip.M_MAX_ABS] == (float(e.max()) if e.numel() else 0.0) or e.numel() == 0
    p64 = pred.double()[1:1 + n].clone().requires_grad_(True)
    both = mask & (gt[3:3 + n] > 0) & (pred[1:1 + n] > 0)
    if int(both.sum()) == 0:
      assert bool(torch.isnan(out['loss'])) or float(out['loss']) == 0.0
      return
    l = torch.log(p64[both]) - torch.log(gt.double()[3:3 + n][both])
    ref = (l * l).mean() - 0.5 * l.mean() ** 2
    ref.backward()
    assert abs(float(out['loss']) - float(ref)) <= 1e-6 * max(abs(float(ref)), float((l * l).mean()))
    assert float((out['gp'].double() - p64.grad).norm()) <= 1e-6 * float(p64.grad.norm())

  return run, verify


for _n in (1, 1023, 4097):
  case('metrics', ['mode_masked_metrics', 'mode_silog_loss_fwd', 'mode_silog_loss_bwd'], b_metrics, (_n,))


def b_erp_metrics(H, W, frames):
  """test_gpu_panorama.test_against_float64_on_the_cpu (8 x the distance of torch CPU fp32 from float64) and the bicubic bound."""
  import panorama_ref as R
  from utils import geometry as HG
  pred, gt = R.make_inputs(frames, H, W, 2023)
  xs = torch.rand(1, 3, 25, 13, generator=torch.Generator().manual_seed(17 + 25 + 3)) * 50  # (test_bicubic_up2_against_float64_interpolate's odd size)

  def run():
    _fresh_caches()
    stats, pe, ge = HF.erp_depth_metrics(P(pred), P(gt), HG._c2e_grid(W, H, DEV), R.MAXDEPTH, ratio=R.RATIOS, return_erp=True)
    return {'stats': stats, 'pe': pe, 'ge': ge, 'up': HF.bicubic_up2(P(xs))}

  def verify(out):
    ge64 = R.c2e(gt, torch.float64)
    assert int(((ge64 - R.MAXDEPTH).abs() <= 1e-4 * R.MAXDEPTH).sum()) == 0
    truth, pe64, _ = R.reference_rows(pred, gt, torch.float64)
    ref32, _, _ = R.reference_rows(pred, gt, torch.float32)
    stats = out['stats'].numpy()
    for f in range(frames):
      assert stats[f][0] == int((ge64[f] <= R.MAXDEPTH).sum())
      ours = R.stat_means(stats[f])
      for k in range(5):
        t = truth[f][k]
        print('  frame %d %s: ours %.3e, torch fp32 %.3e from float64' % (f, R.NAMES[k], abs(ours[k] - t), abs(ref32[f][k] - t)))
        assert abs(ours[k] - t) <= 8 * abs(ref32[f][k] - t), (f, R.NAMES[k])
    close(out, 'pe', pe64, 2e-6 * float(pe64.abs().max()), scale=False)  # test_hip_reprojections: float32 bilinear weights
    t64 = F.interpolate(xs.double(), scale_factor=[2, 2], mode='bicubic', align_corners=True)
    t32 = F.interpolate(xs, scale_factor=[2, 2], mode='bicubic', align_corners=True)
    assert float((out['up'].double() - t64).abs().max()) <= 4 * float((t32.double() - t64).abs().max())

  return run, verify


case('erp_metrics', ['mode_erp_depth_metrics', 'mode_bicubic_up2'], b_erp_metrics, (50, 25, 1))
case('erp_metrics', ['mode_erp_depth_metrics', 'mode_bicubic_up2'], b_erp_metrics, (50, 25, 3))
case('erp_metrics', ['mode_erp_depth_metrics', 'mode_bicubic_up2'], b_erp_metrics, (26, 13, 3))


# ============================================================================================================ geometry, multiview
def b_geometry():
  """disp2depth for a direct, a rotated and a re-projected pair (test_hip_disp2depth); the fused view transform, projection and
  z-buffer on the 64 x 32 golden depth map under the golden poses (tests/golden/geometry.npz): test_hip_fused_view_transform_generic_
  pose_is_the_reference, test_hip_projection, and fused == project + zbuffer of test_hip_view_transform_full_size."""
  from oracle import geometry_ref as G
  from utils import geometry as HG
  z = np.load(os.path.join(GOLDEN, 'geometry.npz'), allow_pickle=False)
  depth, conf = z['a/depth'].astype(np.float32), z['a/conf'].astype(np.float32)
  H, W = depth.shape
  poses = {name: z['a/%s/args' % name].tolist() for name in ('tgen', 't23', 't24', 't34')}
  rng = np.random.RandomState(11)
  disp = rng.rand(H, W).astype(np.float32) * 20
  disp[rng.rand(H, W) < 0.1] = 0

  def run():
    _fresh_caches()
    out = {}
    d, c = P(torch.from_numpy(disp)), P(torch.from_numpy(conf))
    for pair in ('12', '13', '23'):
      out['d' + pair], out['c' + pair] = HG.disp2depth_gpu(d, c, pair)
    dd = P(torch.from_numpy(depth))
    for name, pose in poses.items():
      out['v_' + name], out['k_' + name] = HG.depthViewTransWithConf_gpu(dd, c, *pose)
      r2, tgt = HG.project_gpu(dd, *pose)
      out['r2_' + name], out['tgt_' + name] = r2, tgt
      out['v2_' + name], out['k2_' + name] = HG.zbuffer_gpu(r2, tgt, c)
    return out

  def verify(out):
    rd, rc = G.disp2depth(disp, conf, '12', 'Deep360')
    far = rd >= 999
    assert np.allclose(out['d12'].numpy()[~far], rd[~far], rtol=2e-5, atol=1e-5) and np.array_equal(out['c12'].numpy(), conf)
    rd, rc = G.disp2depth(disp, conf, '13', 'Deep360')
    assert np.median(np.abs(out['d13'].numpy() - rd)) < 1e-4 and np.abs(out['c13'].numpy() - rc).max() < 1e-5
    rd, rc = G.disp2depth(disp, conf, '23', 'Deep360')
    assert abs((out['d23'].numpy() > 0).mean() - (rd > 0).mean()) < 0.05
    for name, pose in poses.items():
      assert torch.equal(out['v_' + name], out['v2_' + name]) and torch.equal(out['k_' + name], out['k2_' + name]), name
      r2_ref, I, J, fi, fj = G.project(depth, *pose)
      live = (depth > 0) & (r2_ref < 100000) & (r2_ref > 0)
      r2, tgt = out['r2_' + name].numpy(), out['tgt_' + name].numpy()
      assert np.array_equal(tgt >= 0, live), name
      assert np.abs(r2[live] - r2_ref[live]).max() <= 1e-12 * r2_ref[live].max(), name
    bad = (out['v_tgen'].numpy() != z['a/tgen/view']) | (out['k_tgen'].numpy() != z['a/tgen/conf'])
    assert bad.sum() <= 1, int(bad.sum())  # a generic pose has no systematic rounding ties

  return run, verify


case('geometry', ['mode_disp2depth', 'mode_grid_sample_border', 'mode_depth_view_trans', 'mode_depth_view_project', 'mode_zbuffer'], b_geometry)


def b_multiview(F_):
  """test_gpu_multiview: the hand-off equals six disp2depth_gpu calls + the interleave bit for bit."""
  from utils import geometry as HG
  H, W = 64, 32
  rng = np.random.RandomState(21 + F_)
  disp = torch.from_numpy(rng.rand(F_, 6, H, W).astype(np.float32) * 20)
  disp[torch.from_numpy(rng.rand(F_, 6, H, W) < 0.1)] = 0
  conf = torch.from_numpy(rng.rand(F_, 6, H, W).astype(np.float32))

  def run():
    _fresh_caches()
    d, c = P(disp), P(conf)
    out = {'frames': HG.disp2depth_frames_gpu(d, c), 'png': HG.disp2depth_frames_gpu(d, c, conf_png=True),
           'depth': HG.disp2depth_frames_gpu(d, c, depth_only=True)}
    singles = []
    for f in range(F_):
      for p, pair in enumerate(HG.PAIRS):
        singles += list(HG.disp2depth_gpu(d[f, p].contiguous(), c[f, p].contiguous(), pair))
    out['singles'] = torch.stack(singles).view(F_, 12, H, W)
    return out

  def verify(out):
    assert torch.equal(out['frames'], out['singles']) and torch.equal(out['depth'], out['frames'][:, 0::2])
    q = torch.from_numpy(HG.conf_png_np(out['singles'][:, 1::2].numpy()))  # the reference's 8-bit export read back, bit for bit
    assert torch.equal(out['png'][:, 0::2], out['frames'][:, 0::2]) and torch.equal(out['png'][:, 1::2], q)

  return run, verify


for _f in (1, 3):
  case('multiview', ['mode_multiview_handoff'], b_multiview, (_f,))


# ============================================================================================================ whole paths
def _train_step():
  """The (32, 128, 64) setup of test_gpu_repeat._net_and_batch: forward + backward; losses and gradients returned."""
  import test_gpu_repeat as R
  import two_rank_worker as trw
  from mode_hip import data_parallel

  def run():
    _fresh_caches()
    net, left, right, gt = R._net_and_batch(32, 128, 64)
    left, right, gt = GB.place(left), GB.place(right), GB.place(gt)  # (a third of gt is NaN: finiteness is asserted by verify)
    red = data_parallel.GradAllReducer(net, fuse_accumulation=True)
    count = data_parallel.global_valid_count(~torch.isnan(gt))
    red.zero_grad()
    loss = trw.step_loss(net, left, right, gt, count)
    loss.backward()
    torch.cuda.synchronize()
    out = {'loss': loss.detach().clone(), 'flat': red.flat.detach().clone()}
    red.detach()
    return out

  def verify(out):
    assert bool(torch.isfinite(out['loss']).all()) and bool(torch.isfinite(out['flat']).all())
    assert float(out['flat'].abs().sum()) > 0

  return run, verify


def _eval_forward():
  import test_gpu_repeat as R

  def run():
    _fresh_caches()
    net, left, right, gt = R._net_and_batch(32, 128, 64)
    left, right = GB.place(left), GB.place(right)
    bns = [m for m in net.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)]
    for m in bns:
      m.momentum = 1.0  # running statistics := this batch's, as in test_eval_forward_launches_no_batchnorm_kernel: eval mode as well
    with torch.no_grad():  # conditioned as train mode (with the state's own running statistics the logits overflow)
      net(left, right)
    net.eval()
    with torch.no_grad():
      pred = net(left, right)
      again = net(left, right)  # the second forward runs on the packed weights the first one kept (mode_weight_pack_reuse)
    return {'pred': pred, 'again': again}

  def verify(out):
    assert out['pred'].shape[-2:] == (128, 64) and float(out['pred'].min()) >= 0 and float(out['pred'].max()) <= 31
    assert torch.equal(out['again'], out['pred'])

  return run, verify


def _fusion_forward():
  """ModeFusion at the golden tiny size, train-mode forward + backward and eval forward, against test_fusion's golden bound."""
  import test_fusion as TF
  from models import mode_fusion
  from oracle import fusion_ref
  z = np.load(os.path.join(GOLDEN, 'fusion_tiny.npz'), allow_pickle=False)
  maxdepth, channels, manifest, sd, depthes, confs, rgbs, gt = TF._case(z)

  def run():
    _fresh_caches()
    net = mode_fusion.ModeFusion(maxdepth, channels, {'depth': 12, 'rgb': 12}).to(DEV)
    net.load_state_dict(sd)
    dd, cc, rr = [P(t) for t in depthes], [P(t) for t in confs], [P(t) for t in rgbs]
    net.train()
    pred = net(dd, cc, rr)
    loss = fusion_ref.training_loss(pred, P(gt), maxdepth)
    loss.backward()
    grads = [p.grad.detach().clone() for p in net.parameters()]
    net.eval()
    with torch.no_grad():
      ev = net(dd, cc, rr)
    return {'train': pred.detach(), 'loss': loss.detach(), 'eval': ev, 'grads': grads}

  def verify(out):
    for name in ('train', 'eval'):  # the bound of test_fusion.test_gpu_fusion_train_and_eval
      truth, ref32 = z['truth64/%s_pred' % name], z['%s/pred' % name]
      err, ref_err = np.abs(out[name].numpy().astype(np.float64) - truth), np.abs(ref32 - truth)
      assert err.max() <= max(1e-4, 3 * ref_err.max()) and err.mean() <= max(1e-6, 2 * ref_err.mean()), (name, err.max(), ref_err.max())
    assert abs(float(out['loss']) - float(z['train/loss'])) < 1e-4 * float(z['train/loss'])

  return run, verify


TRAIN_STEP_ENTRIES = []
EVAL_ENTRIES = []
FUSION_ENTRIES = []
case('path_train_step', TRAIN_STEP_ENTRIES, _train_step)
case('path_eval_forward', EVAL_ENTRIES, _eval_forward)
case('path_fusion', FUSION_ENTRIES, _fusion_forward)


# ============================================================================================================ the test
def run_case(c, monkeypatch):
  real = mode_hip.lib()
  rec = RecordingLib(real)
  for k, v in c.switches.items():
    assert hasattr(HF, k), k
    monkeypatch.setattr(HF, k, v)
  prev = HF.CONV_ARITH
  if c.arith:
    HF.set_conv_arith(c.arith)
  monkeypatch.setattr(mode_hip, '_lib', rec)
  try:
    run, verify = c.build(*c.args)
    leaves, stats = GB.under_two_fills(run)
  finally:
    monkeypatch.setattr(mode_hip, '_lib', real)
    HF.set_conv_arith(prev)
  out = {}
  for path, t in leaves:  # "out['y']" -> y; "out['g'][2]" -> g[2]
    key = path[len("out['"):].replace("']", '', 1)
    out[key] = t
  verify(out)
  return rec, stats


@pytest.fixture(autouse=True)
def _stop_at_a_gpu_fault():
  """A fault is a finding, not something to run into again: if the device no longer answers after a test, the session ends there."""
  yield
  try:
    torch.cuda.synchronize()
  except RuntimeError as e:
    pytest.exit('the GPU reported an error after this test; nothing more is started on it: %s' % e, returncode=3)


@pytest.mark.parametrize('c', CASES, ids=[c.id for c in CASES])
def test_guarded(c, monkeypatch):
  rec, stats = run_case(c, monkeypatch)
  assert c.entries, 'every case declares the entries it is there to launch'
  missing = sorted(c.entries - set(rec.launched))
  assert not missing, 'declared but not launched: %s (launched: %s)' % (missing, sorted(rec.launched))
  STATS['allocations'] += sum(stats['allocations'])
  STATS['launches'] += sum(rec.launched.values())
  STATS['cases'] += 1
  print('  %d guarded allocations, %d launching calls' % (sum(stats['allocations']), sum(rec.launched.values())))
  print('LAUNCHED %s %s' % (c.id, ' '.join(sorted(rec.launched))))


class _Twice(torch.autograd.Function):

  @staticmethod
  def forward(ctx, x):
    return x * 2

  @staticmethod
  def backward(ctx, g):
    ws = HF.abs_max(g)  # allocates its result buffer from mode_hip/functional.py, on the engine's device thread
    _Twice.seen.append(ws)
    return g * 2


def test_allocations_inside_a_backward_on_the_device_thread_are_guarded():
  """The dispatch mode is thread-local state that the autograd engine hands to its device thread: a buffer that the host code
  allocates inside a Function.backward lies between guards too."""
  import threading
  _Twice.seen = []
  main = threading.get_ident()
  threads = []

  class Probe(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x):
      return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
      threads.append(threading.get_ident())
      return g

  with GB.guarded(0) as gb:
    x = GB.place(_rand((3, 5), 1).to(DEV)).requires_grad_(True)
    n0 = len(gb.allocations)
    _Twice.apply(Probe.apply(x)).sum().backward()
    torch.cuda.synchronize()
    assert threads and threads[0] != main, 'backward of a CUDA graph runs on the device thread'
    made = gb.allocations[n0:]
    assert made and all(a.where.startswith('mode-2022_amd/mode_hip/functional.py:') for a in made), [a.describe() for a in made]
    ptrs = {a.block.data_ptr() + a.front for a in made}
    assert _Twice.seen[0].data_ptr() in ptrs
    gb.check()


def test_zz_report():
  """What the run saw (for the record; `-s` shows it)."""
  print('guard bands: %(cases)d cases, %(allocations)d guarded allocations, %(launches)d launching calls' % STATS)
