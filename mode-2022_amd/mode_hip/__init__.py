"""ctypes binding of libmode_hip.so, derived from include/mode_hip.h: the header that declares the C-ABI is read (_header.py) and every
signature, constant and record here is what it says -- nothing of it is written a second time.

This is the only place that touches the native library.  There is NO fallback: if the library is
missing or a tensor is not on a GPU, the call raises.  PyTorch is used for device memory and
streams only (tensor.data_ptr(), torch.cuda.current_stream()).
"""
import ctypes
import os
import threading

import torch

from . import _header

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, 'libmode_hip.so')

HEADER = _header.load()  # include/mode_hip.h, read once: the prototypes, constants and records below are its own
PROTOTYPES = HEADER.prototypes  # name -> (return C type, [(C type, parameter name)])
SIGNATURES = HEADER.signatures  # name -> (restype, argtypes) as ctypes classes
LAUNCHING = frozenset(n for n, (_, params) in PROTOTYPES.items() if any(t == _header.STREAM for t, _ in params))  # enqueue work on a stream
CONSTANTS = HEADER.constants  # every MODE_* integer of the header, under the header's name

ABI_VERSION = CONSTANTS['MODE_HIP_ABI_VERSION']

# The extension headers, read the same way.  A public header is frozen once its tests pin what it holds (the first; the second with
# its version and its four launching entries), so entries added since are declared in a header of their own and bound onto the same
# handle.  Per header (NAME, file, version constant, version function) the module gets NAME (the header), NAME_LAUNCHING and
# NAME_VERSION; HEADER, SIGNATURES, ... above stay the first header's.  The next header is one more row.
EXTENSIONS = (('SELFSUP', 'mode_hip_selfsup.h', 'MODE_SELFSUP_VERSION', 'mode_selfsup_version'),
              ('MVPHOTO', 'mode_hip_mvphoto.h', 'MODE_MVPHOTO_VERSION', 'mode_mvphoto_version'),
              ('MVPOSE', 'mode_hip_mvpose.h', 'MODE_MVPOSE_VERSION', 'mode_mvpose_version'))
# EXTENSIONS is pinned to those three rows by the fourth header's tests; the rows since stand in a second tuple that the same two
# loops walk after the first.  The next header is one more row here.
EXTENSIONS_2 = (('MVVIS', 'mode_hip_mvvis.h', 'MODE_MVVIS_VERSION', 'mode_mvvis_version'),)
# EXTENSIONS_2 is pinned to that row by the fifth header's tests in its turn: a third tuple, the same two loops.
EXTENSIONS_3 = (('MVRENDER', 'mode_hip_mvrender.h', 'MODE_MVRENDER_VERSION', 'mode_mvrender_version'),)
for _name, _file, _const, _ in EXTENSIONS + EXTENSIONS_2 + EXTENSIONS_3:
  _h = _header.load(os.path.join(os.path.dirname(_header.PATH), _file))
  globals().update({_name: _h, _name + '_VERSION': _h.constants[_const], _name + '_LAUNCHING': frozenset(
      n for n, (_, params) in _h.prototypes.items() if any(t == _header.STREAM for t, _ in params))})
_lib = None
_lock = threading.Lock()


def lib():
  """Load (once) and return the native library; raises if it has not been built."""
  global _lib
  if _lib is None:
    with _lock:
      if _lib is None:
        if not os.path.exists(LIB_PATH):
          raise RuntimeError('libmode_hip.so is not built (%s missing): run `python -c "import __graft_entry__ as g; '
                             'g.build()"` or `python mode-2022_amd/mode_hip/build.py`' % LIB_PATH)
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
          fn = getattr(handle, name)
          fn.restype = res
          fn.argtypes = args
        have = handle.mode_hip_abi_version()
        if have != ABI_VERSION:
          raise RuntimeError('libmode_hip.so has ABI version %d, this binding needs %d: rebuild it (python '
                             'mode-2022_amd/mode_hip/build.py)' % (have, ABI_VERSION))
        for ext, file, _, version_fn in EXTENSIONS + EXTENSIONS_2 + EXTENSIONS_3:
          have = getattr(handle, version_fn)() if hasattr(handle, version_fn) else None
          want = globals()[ext + '_VERSION']  # read now, not at import
          if have != want:
            raise RuntimeError('libmode_hip.so has version %s of the entries of %s, this binding needs %d: rebuild it '
                               '(python mode-2022_amd/mode_hip/build.py)' % (have, file, want))
          for name, (res, args) in globals()[ext].signatures.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
  return _lib


BnEpilogue = _header.structure(HEADER, 'mode_bn_epilogue', 'BnEpilogue', 'struct mode_bn_epilogue (host-side struct of device pointers).')

# indices into the statistic vector of mode_masked_metrics / mode_silog_loss_fwd
METRICS_MAX_THRESHOLDS, METRICS_COUNT = CONSTANTS['MODE_METRICS_MAX_THRESHOLDS'], CONSTANTS['MODE_METRICS_COUNT']
(M_N, M_N_GT, M_N_BOTH, M_SUM_ABS, M_SUM_SQ, M_SUM_ABSREL, M_SUM_SQREL, M_SUM_LOG, M_SUM_LOG2, M_MAX_ABS, M_PX, M_D1, M_RATIO) = (
    CONSTANTS['MODE_METRICS_' + k] for k in 'N N_GT N_BOTH SUM_ABS SUM_SQ SUM_ABSREL SUM_SQREL SUM_LOG SUM_LOG2 MAX_ABS PX D1 RATIO'.split())
MetricsParams = _header.structure(HEADER, 'mode_metrics_params', 'MetricsParams', 'struct mode_metrics_params (host memory, read during the call).')

# the statistics of one disparity map as mode_photometric_loss_fwd leaves them
PHOTOMETRIC_MAX_MAPS, PHOTOMETRIC_STATS = CONSTANTS['MODE_PHOTOMETRIC_MAX_MAPS'], CONSTANTS['MODE_PHOTOMETRIC_STATS']
(PH_N_VALID, PH_SUM_PE, PH_SUM_SMOOTH_X, PH_SUM_SMOOTH_Y) = (CONSTANTS['MODE_PHOTOMETRIC_' + k] for k in 'N_VALID SUM_PE SUM_SMOOTH_X SUM_SMOOTH_Y'.split())
PhotometricParams = _header.structure(HEADER, 'mode_photometric_params', 'PhotometricParams',
                                      'struct mode_photometric_params (host memory, read during the call).')

# left-right consistency: the statistics of one view and map as mode_lr_consistency_fwd leaves them
LR_STATS = SELFSUP.constants['MODE_LR_STATS']
(LR_N_VALID, LR_SUM_E, LR_N_VISIBLE) = (SELFSUP.constants['MODE_LR_' + k] for k in 'N_VALID SUM_E N_VISIBLE'.split())
LrParams = _header.structure(SELFSUP, 'mode_lr_params', 'LrParams', 'struct mode_lr_params (host memory, read during the call).')

# multi-view reprojection loss: the statistics as mode_mvphoto_loss_fwd leaves them
MVP_MAX_SOURCES, MVP_STATS, MVP_NO_WINNER = (MVPHOTO.constants['MODE_MVP_' + k] for k in 'MAX_SOURCES STATS NO_WINNER'.split())
(MVP_N, MVP_SUM_MIN, MVP_SUM_SMOOTH_X, MVP_SUM_SMOOTH_Y, MVP_WINS) = (MVPHOTO.constants['MODE_MVP_' + k] for k in 'N SUM_MIN SUM_SMOOTH_X SUM_SMOOTH_Y WINS'.split())

# novel-view rendering: the colour modes, and the classes of a target pixel as mode_mv_render leaves them in hit
MVR_SPLAT, MVR_RESAMPLE, MVR_MAX_CHANNELS = (MVRENDER.constants['MODE_MVR_' + k] for k in 'SPLAT RESAMPLE MAX_CHANNELS'.split())
(MVR_HIT_NONE, MVR_HIT_DIRECT, MVR_HIT_FILLED, MVR_HIT_RESAMPLED) = (MVRENDER.constants['MODE_MVR_HIT_' + k] for k in 'NONE DIRECT FILLED RESAMPLED'.split())


def check(rc, what):
  if rc != 0:
    msg = lib().mode_last_error()
    raise RuntimeError('%s failed (code %d): %s' % (what, rc, msg.decode() if msg else ''))


def ptr(t):
  return ctypes.c_void_p(t.data_ptr())


def stream_of(t):
  return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def require_gpu(*tensors):
  """Same refusal as the reference op (sphere_conv.py:33-34): no CPU path exists."""
  for t in tensors:
    if t is not None and not t.is_cuda:
      raise NotImplementedError('Only support cuda tensor!')


def require_f32c(*tensors):
  for t in tensors:
    if t.dtype != torch.float32:
      raise TypeError('libmode_hip kernels are fp32 (got %s)' % t.dtype)
    if not t.is_contiguous():
      raise ValueError('libmode_hip kernels need contiguous tensors')
