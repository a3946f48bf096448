#!/usr/bin/env python3
"""What the host code of the regular 3x3 Conv2d family answered at the commit BEFORE csrc/conv2d.hip became pure host code with one
argument check (conv2d_f32_fwd.hip, conv2d_f32_wgrad.hip and conv2d.hip): no GPU needed, nothing is launched.

  python tests/golden/make_golden_conv2d_host.py     # writes conv2d_parent_host.json

conv2d_parent_host.json holds
  queries   the four pure host functions whose bodies moved, over GRID: mode_conv2d_wpack_bytes and
            mode_conv2d_bwd_weight_workspace_bytes as lists of integers, mode_conv2d_split_supported and
            mode_conv2d_split_shape_supported as strings of 0 / 1, each in the order queries() walks the grid;
  refusals  {case: return code} of calls that are wrong in exactly ONE way, over the family's twelve compute entries and
            mode_zero_insert2: a zero size, dilation 3, a sample of 2^29 elements, 129 rows (fp32 forward / input gradient), channel
            counts off the split kernels' grid, each pointer null in turn, and each entry's own rules (a null maximum, a null epilogue
            or a null vector in it, a null acc, acc that is the output, an odd width or unaligned tensors for the zero insertion).
            Every such call is refused before a launch; calls with an empty batch are not here -- they need a stream.
tests/test_conv2d_args_host.py asserts that the tree gives the same values and codes, and that every refusal's message names its
entry.  Calls that are wrong in two ways are not covered: the one check order of conv2d.hip may refuse them for the other reason."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, 'mode-2022_amd')):
  if p not in sys.path:
    sys.path.insert(0, p)

OUT = os.path.join(HERE, 'conv2d_parent_host.json')

CHANNELS = (1, 8, 16, 20, 32, 40, 64, 96, 128, 256, 512, 528)
PLANES = ((7, 33), (128, 512), (1024, 512), (2048, 4096))
BATCHES = (1, 4)
DILATIONS = (1, 2, 3)
WHICH = (0, 1, 2, 3)


def queries(lib):
  pairs = [(ci, co) for ci in CHANNELS for co in CHANNELS]
  return {
      'wpack_bytes': [lib.mode_conv2d_wpack_bytes(ci, co) for ci, co in pairs],
      'bwd_weight_workspace_bytes': [lib.mode_conv2d_bwd_weight_workspace_bytes(b, ci, h, w, co)
                                     for ci, co in pairs for h, w in PLANES for b in BATCHES],
      'split_supported': ''.join(str(lib.mode_conv2d_split_supported(ci, co, d, k)) for ci, co in pairs for d in DILATIONS for k in WHICH),
      'split_shape_supported': ''.join(str(lib.mode_conv2d_split_shape_supported(ci, co, h, w, d, k))
                                       for ci, co in pairs for h, w in PLANES for d in DILATIONS for k in WHICH),
  }


# entry: (pointer arguments in order, 'bn' = the epilogue; trailing integers after (B, Ci, H, W, Co, dilation)), split `which` or None
ENTRIES = {
    'mode_conv2d_fwd': (('x', 'w', 'y', 'wpack'), (), None),
    'mode_conv2d_bwd_data': (('gy', 'w', 'gx', 'wpack'), (), None),
    'mode_conv2d_fwd_bn': (('x', 'w', 'bn', 'y', 'wpack'), (), None),
    'mode_conv2d_bwd_weight': (('gy', 'x', 'gw', 'workspace'), (0,), None),
    'mode_conv2d_fwd_split': (('x', 'w', 'bn', 'y', 'wpack'), (), 0),
    'mode_conv2d_bwd_data_split': (('gy', 'w', 'gx', 'wpack'), (), 1),
    'mode_conv2d_bwd_data_split_acc': (('gy', 'w', 'acc', 'gx', 'wpack'), (), 1),
    'mode_conv2d_fwd_split_f16': (('x', 'w', 'amax_x', 'amax_w', 'y', 'wpack'), (), 0),
    'mode_conv2d_bwd_data_split_f16': (('gy', 'w', 'amax_g', 'amax_w', 'acc', 'gx', 'wpack'), (), 1),
    'mode_conv2d_fwd_split_f16_bn': (('x', 'w', 'amax_x', 'bn', 'y', 'amax_y', 'wpack'), (), 0),
    'mode_conv2d_bwd_weight_split': (('gy', 'x', 'gw', 'workspace'), (0,), 2),
    'mode_conv2d_bwd_weight_split_f16': (('gy', 'x', 'amax_g', 'amax_x', 'gw', 'workspace'), (0,), 2),
}
OPTIONAL = {('mode_conv2d_fwd_split', 'bn'), ('mode_conv2d_bwd_data_split_f16', 'acc')}  # NULL is a valid value there
SHAPE = dict(B=1, Ci=32, H=8, W=32, Co=32, dilation=1)


def refusal_cases():
  """[(case id, entry, {pointer name: value | None}, shape dict)] -- never a call that would be accepted."""
  out = []
  for name, (ptrs, _, which) in ENTRIES.items():
    def add(tag, shape=None, **nulls):
      out.append(('%s/%s' % (name, tag), name, nulls, dict(SHAPE, **(shape or {}))))
    for size in ('Ci', 'H', 'W', 'Co'):
      add('zero_' + size, {size: 0})
    add('negative_B', {'B': -1})
    add('dilation_3', {'dilation': 3})
    add('sample_2^29', {'H': 1 << 12, 'W': 1 << 12})  # 32 channels * 2^24 pixels
    if which is None and name != 'mode_conv2d_bwd_weight':
      add('129_rows', {'Ci' if name == 'mode_conv2d_bwd_data' else 'Co': 129})
    if which in (0, 1):
      add('reduction_off_16', {'Co' if which else 'Ci': 24})
      add('one_row', {'Ci' if which else 'Co': 1})
      add('513_rows', {'Ci' if which else 'Co': 513})
    for p in ptrs:
      if (name, p) not in OPTIONAL:
        add('null_' + p, **{p: None})
    if 'bn' in ptrs:
      for vec in ('gamma', 'beta', 'mean', 'var'):
        add('bn_null_' + vec, bn_null=vec)
    if 'acc' in ptrs:
      add('acc_is_gx', acc='gx')
  for tag, kw in (('zero_Ho', dict(Ho=0)), ('zero_Wo', dict(Wo=0)), ('negative_planes', dict(planes=-1)), ('odd_Wo', dict(Wo=7)),
                  ('null_in', dict(inp=0)), ('null_out', dict(out=0)), ('unaligned_in', dict(inp=20)), ('unaligned_out', dict(out=24))):
    out.append(('mode_zero_insert2/' + tag, 'mode_zero_insert2', kw, None))
  return out


def call(lib, case):
  """(return code, message) of one refusal case."""
  from mode_hip import BnEpilogue
  _, name, nulls, shape = case
  null = ctypes.c_void_p(0)
  if name == 'mode_zero_insert2':
    a = dict(inp=64, out=128, planes=2, Ho=4, Wo=8)
    a.update(nulls)
    rc = lib.mode_zero_insert2(ctypes.c_void_p(a['inp']), ctypes.c_void_p(a['out']), a['planes'], a['Ho'], a['Wo'], null)
    return rc, lib.mode_last_error()
  ptrs, tail, _ = ENTRIES[name]
  addr = {p: 64 * (i + 1) for i, p in enumerate(ptrs)}  # distinct fake addresses: no call here gets as far as reading one
  vecs = {v: ctypes.c_void_p(4096 + 64 * i) for i, v in enumerate(('gamma', 'beta', 'mean', 'var'))}
  if 'bn_null' in nulls:
    vecs[nulls['bn_null']] = null
  e = BnEpilogue(vecs['gamma'], vecs['beta'], vecs['mean'], vecs['var'], 1e-5, None, 1)
  args = []
  for p in ptrs:
    v = nulls.get(p, p)
    if v is None:
      args.append(None if p == 'bn' else null)
    elif p == 'bn':
      args.append(ctypes.byref(e))
    else:
      args.append(ctypes.c_void_p(addr[v]))  # (v != p: acc given the address of gx)
  s = shape
  rc = getattr(lib, name)(*args, s['B'], s['Ci'], s['H'], s['W'], s['Co'], s['dilation'], *tail, null)
  return rc, lib.mode_last_error()


def main():
  import mode_hip
  lib = mode_hip.lib()
  refusals = {}
  for case in refusal_cases():
    rc, msg = call(lib, case)
    assert rc < 0 and case[1].encode() in msg, (case[0], rc, msg)
    refusals[case[0]] = rc
  with open(sys.argv[1] if len(sys.argv) > 1 else OUT, 'w') as f:
    json.dump({'queries': queries(lib), 'refusals': refusals}, f, indent=0, sort_keys=True)
    f.write('\n')
  print('%d refusals, %s query values' % (len(refusals), {k: len(v) for k, v in queries(lib).items()}))


if __name__ == '__main__':
  main()
