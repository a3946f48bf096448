"""CPU: mode_hip/_header.py, the reader that derives the ctypes binding from include/mode_hip.h -- each construct on a small synthetic
header, and the real header against signatures written out here by hand (so that the reader does not certify itself)."""
import ctypes

import pytest

import mode_hip
from mode_hip import _header

I, P, F, LL, SZ = ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_longlong, ctypes.c_size_t


def _one(text):
  h = _header.parse(text)
  (name, proto), = h.prototypes.items()
  return name, proto, h.signatures[name]


@pytest.mark.parametrize('c_type,want', [('int', I), ('int32_t', I), ('unsigned', ctypes.c_uint), ('long long', LL), ('size_t', SZ), ('float', F),
                                         ('double', ctypes.c_double), ('mode_stream_t', P), ('const float*', P), ('void*', P), ('int64_t*', P)])
def test_every_type_of_the_map(c_type, want):
  name, proto, (res, args) = _one('int f(%s a, %s);' % (c_type, c_type))
  assert name == 'f' and proto == ('int', [(c_type, 'a'), (c_type, '')])  # the second parameter is unnamed
  assert res is I and len(args) == 2 and args[0] is want and args[1] is want


def test_return_types():
  assert _one('size_t f(int n);')[2] == (SZ, [I])
  assert _one('const char* f(void);')[1:] == (('const char*', []), (ctypes.c_char_p, []))
  assert _one('int f();')[2] == (I, [])
  assert _one('int f(const char* s);')[2][1][0] is P  # c_char_p is for the RETURN only


def test_pointers():
  name, proto, sig = _one('int f(const float* const* pp, const long long *sizes, const mode_thing* rec, float * * q);')
  assert proto[1] == [('const float* const*', 'pp'), ('const long long*', 'sizes'), ('const mode_thing*', 'rec'), ('float**', 'q')]
  assert sig[1] == [P] * 4 and all(a is P for a in sig[1])


def test_a_prototype_over_several_lines_and_comments():
  text = '''/* int mode_quoted(int a, mode_stream_t s); in prose, like mode_pack_reuse(1) */
  // int mode_slashed(int a);
  int mode_real(const float* x,   /* the input */
                long long n, int which /* 0 forward, 1 backward */,
                mode_stream_t stream);
  '''
  h = _header.parse(text)
  assert list(h.prototypes) == ['mode_real']
  assert h.prototypes['mode_real'] == ('int', [('const float*', 'x'), ('long long', 'n'), ('int', 'which'), ('mode_stream_t', 'stream')])
  assert h.signatures['mode_real'][1] == [P, LL, I, P]


def test_an_unknown_type_names_the_entry():
  with pytest.raises(TypeError, match=r"mode_odd.*'short'"):
    _header.parse('int mode_fine(int a);\nint mode_odd(int a, short b);')
  with pytest.raises(TypeError, match=r"mode_ret.*'bool'"):
    _header.parse('bool mode_ret(int a);')
  with pytest.raises(TypeError, match='mode_by_value'):  # a record by value is not in the map either
    _header.parse('int mode_by_value(mode_thing t);')
  with pytest.raises(ValueError, match='does not know'):
    _header.parse('int f(int a);\nstatic int g = 3;')
  with pytest.raises(ValueError, match='twice'):
    _header.parse('int f(int a);\nint f(int a);')


def test_constants():
  text = '''#ifndef MODE_GUARD_H_
  #define MODE_GUARD_H_
  enum { MODE_OK = 0, MODE_ERR_A = -1, /* why */ MODE_ERR_B = -2 };
  #define MODE_N 4 /* a comment */
  #define MODE_HEX 0x10
  #define MODE_A 10
  #define MODE_B (MODE_A + MODE_N)
  #define MODE_C (MODE_B + 2 * MODE_N - 1)
  #define OTHER_THING 7
  #endif'''
  assert _header.parse(text).constants == {'MODE_OK': 0, 'MODE_ERR_A': -1, 'MODE_ERR_B': -2, 'MODE_N': 4, 'MODE_HEX': 16, 'MODE_A': 10,
                                           'MODE_B': 14, 'MODE_C': 21}
  with pytest.raises(ValueError, match='MODE_LATE'):
    _header.parse('#define MODE_LATE (MODE_LATER + 1)\n#define MODE_LATER 1')
  with pytest.raises(ValueError, match='MODE_F'):
    _header.parse('#define MODE_F 1.5f')


def test_records():
  text = '''#define MODE_MAX 4
  typedef void* mode_stream_t; /* not a record */
  typedef struct mode_rec {
    const float* p; /* a pointer */
    float a, b2, c;
    float mean[3], std[3];
    int n;
    long long first;
    float w[MODE_MAX]; // sized by a constant
  } mode_rec;
  int mode_use(const mode_rec* r, mode_stream_t s);'''
  h = _header.parse(text)
  assert h.records == {'mode_rec': [('p', 'const float*', None), ('a', 'float', None), ('b2', 'float', None), ('c', 'float', None), ('mean', 'float', 3),
                                    ('std', 'float', 3), ('n', 'int', None), ('first', 'long long', None), ('w', 'float', 4)]}
  assert list(h.prototypes) == ['mode_use'] and h.signatures['mode_use'] == (I, [P, P])
  S = _header.structure(h, 'mode_rec', 'Rec')
  assert S.__name__ == 'Rec' and [n for n, _ in S._fields_] == ['p', 'a', 'b2', 'c', 'mean', 'std', 'n', 'first', 'w']
  assert S.p.offset == 0 and S.a.offset == 8 and S.mean.offset == 20 and S.n.offset == 44 and S.first.offset == 48 and ctypes.sizeof(S) == 72
  assert S._fields_[0][1] is P and S._fields_[4][1] is F * 3 and S._fields_[7][1] is LL
  with pytest.raises(ValueError, match='mode_bad'):
    _header.parse('typedef struct mode_bad { float *a, *b; } mode_bad;')


def test_a_missing_header_names_its_path(tmp_path):
  with pytest.raises(RuntimeError, match='no_such_header.h'):
    _header.load(str(tmp_path / 'no_such_header.h'))


# ------------------------------------------------------------------------------------------------ the real header
def test_spot_checks_written_out_by_hand():
  S = mode_hip.SIGNATURES
  want = {
      'mode_sum_n': (I, [P, P, P, P, P, LL, P]),
      'mode_masked_metrics': (I, [P, P, P, LL, P, P, SZ, P, P]),
      'mode_smooth_l1_masked': (I, [P, P, P, P, F, F, F, P, P, P, LL, P]),
      'mode_sphere_adjoint_build': (I, [P, I, I, I, I, I, I, I, I, P, P, P]),
      'mode_debug_poison': (I, [ctypes.c_uint, P]),
      'mode_last_error': (ctypes.c_char_p, []),
      'mode_hip_abi_version': (I, []),
      'mode_adam_workspace_bytes': (SZ, [LL]),
      'mode_weight_pack_reuse': (I, [I]),
      'mode_abs_max_batch': (I, [P, P, I, P, P]),
      'mode_multiview_rig_handoff': (I, [P, P, I, I, I, I, P, I, P, P, I, P, I, P, P, P]),
      'mode_bn_eval_fwd': (I, [P, P, P, P, P, P, F, I, P, I, I, LL, P]),
      'mode_disp2depth': (I, [P, P, I, I, F, P]),
  }
  for name, (res, args) in want.items():
    got = S[name]
    assert got[0] is res and len(got[1]) == len(args) and all(a is b for a, b in zip(got[1], args)), (name, got)
  P_ = mode_hip.PROTOTYPES
  assert P_['mode_sphere_adjoint_build'][1][-3:] == [('int32_t*', 'rowptr_host'), ('int32_t*', 'entries_host'), ('int64_t*', 'n_entries')]
  assert P_['mode_masked_metrics'][1][4] == ('const mode_metrics_params*', 'params') and P_['mode_masked_metrics'][1][6][0] == 'size_t'
  assert P_['mode_abs_max_batch'][1][:2] == [('const float* const*', 'device_ptrs'), ('const long long*', 'device_sizes')]
  assert 'mode_pack_reuse' not in S and 'mode_stream_t' not in S  # a name quoted in the prose; the typedef


def test_counts_constants_and_records_of_abi_31():
  assert mode_hip.ABI_VERSION == mode_hip.CONSTANTS['MODE_HIP_ABI_VERSION'] == 31
  assert len(mode_hip.SIGNATURES) == 173 and set(mode_hip.SIGNATURES) == set(mode_hip.PROTOTYPES) and len(mode_hip.CONSTANTS) == 42
  assert all(n.startswith('mode_') for n in mode_hip.SIGNATURES)
  assert [mode_hip.CONSTANTS[k] for k in ('MODE_OK', 'MODE_ERR_BAD_ARG', 'MODE_ERR_UNSUPPORTED', 'MODE_ERR_WORKSPACE')] == [0, -1, -2, -3]
  assert (mode_hip.M_N, mode_hip.M_MAX_ABS, mode_hip.M_PX, mode_hip.M_D1, mode_hip.M_RATIO, mode_hip.METRICS_COUNT) == (0, 9, 10, 14, 18, 22)
  assert mode_hip.METRICS_MAX_THRESHOLDS == 4 and mode_hip.PHOTOMETRIC_MAX_MAPS == 4 and mode_hip.PHOTOMETRIC_STATS == 4
  assert (mode_hip.PH_N_VALID, mode_hip.PH_SUM_PE, mode_hip.PH_SUM_SMOOTH_X, mode_hip.PH_SUM_SMOOTH_Y) == (0, 1, 2, 3)
  assert sorted(mode_hip.HEADER.records) == ['mode_adam_chunk', 'mode_adam_segment', 'mode_bn_epilogue', 'mode_metrics_params', 'mode_mv_pair',
                                             'mode_photometric_params']
  assert [ctypes.sizeof(s) for s in (mode_hip.BnEpilogue, mode_hip.MetricsParams, mode_hip.PhotometricParams)] == [56, 76, 60]
  assert [n for n, _ in mode_hip.BnEpilogue._fields_] == ['gamma', 'beta', 'mean', 'var', 'eps', 'add', 'relu']
  assert [n for n, _ in mode_hip.MetricsParams._fields_] == ['n_px', 'px', 'n_d1', 'd1_px', 'd1_pct', 'n_ratio', 'ratio']
  assert [n for n, _ in mode_hip.PhotometricParams._fields_] == ['alpha', 'lam', 'beta', 'c1', 'c2', 'mean', 'std', 'weights']
  assert mode_hip.PhotometricParams.mean.offset == 20 and mode_hip.PhotometricParams.weights.offset == 44 and mode_hip.BnEpilogue.add.offset == 40


def test_the_records_of_the_optimizer_as_numpy_dtypes():
  import numpy as np
  from mode_hip import optim
  seg = np.dtype([('param', '<u8'), ('first', '<i8'), ('numel', '<i8'), ('group', '<i4'), ('unused', '<i4')])
  chunk = np.dtype([('off', '<i8'), ('seg', '<i4'), ('count', '<i4')])
  for got, want in ((optim.SEGMENT, seg), (optim.CHUNK_RECORD, chunk)):
    assert got == want and got.names == want.names and got.itemsize == want.itemsize
    assert [got.fields[n][:2] for n in got.names] == [want.fields[n][:2] for n in want.names]  # formats and offsets
  assert (optim.CHUNK, optim.STATE_DOUBLES, optim.GROUP_DOUBLES) == (2048, 8, 8)
  assert (optim.S_STEP, optim.S_SKIPPED, optim.S_GRAD_NORM, optim.S_FOUND_INF, optim.S_NONFINITE) == (0, 1, 2, 3, 4)


def test_launching_is_having_a_stream_parameter():
  L = mode_hip.LAUNCHING
  assert isinstance(L, frozenset) and len(L) == 122 and L <= set(mode_hip.SIGNATURES)
  for name, (_, params) in mode_hip.PROTOTYPES.items():
    streams = [i for i, (t, _) in enumerate(params) if t == 'mode_stream_t']
    assert (name in L) == bool(streams)
    if streams:  # exactly one, and it is the last parameter: what the spies of the GPU tests pass to mode_debug_poison
      assert streams == [len(params) - 1] and params[-1][1] == 'stream' and mode_hip.SIGNATURES[name][1][-1] is ctypes.c_void_p
  assert 'mode_abs_max_batch' in L and 'mode_abs_max' in L and 'mode_debug_poison' in L
  host = [n for n in mode_hip.SIGNATURES if n.endswith(('_bytes', '_supported'))]
  assert len(host) > 30 and not L & set(host)
  assert not L & {'mode_weight_pack_reuse', 'mode_hip_abi_version', 'mode_last_error', 'mode_sphere_plan_build', 'mode_sphere_adjoint_build',
                  'mode_conv3d_fwd_split_stats_partials'}

