"""CPU tier: the host side of mode_hip.optim.Adam (mode-2022_amd/mode_hip/optim.py, csrc/optim.hip) -- what the constructor refuses, what
the C entries refuse before any launch, and the chunk table the update kernel walks.  The arithmetic is tested on the GPU
(tests/test_gpu_optim.py); zero_grad(set_to_none=True) keeping the views is tested there too: the constructor needs device memory."""
import ctypes

import numpy as np
import pytest
import torch

import mode_hip
from mode_hip import optim

SIZES = [1, 3, 5, 864, 4097, 4098, 1000]  # the seven tensors of tests/test_gpu_optim.py
GROUPS = [0, 0, 0, 0, 1, 1, 1]


def _param(*shape, **kw):
  return torch.nn.Parameter(torch.zeros(*shape, **kw))


def test_the_constructor_refuses_what_the_kernels_do_not_do():
  with pytest.raises(ValueError, match='amsgrad'):
    optim.Adam([_param(3)], amsgrad=True)
  with pytest.raises(ValueError, match='maximize'):
    optim.Adam([_param(3)], maximize=True)
  with pytest.raises(ValueError, match='amsgrad'):  # also through a parameter group
    optim.Adam([{'params': [_param(3)]}, {'params': [_param(2)], 'amsgrad': True}])
  with pytest.raises(NotImplementedError, match='Only support cuda tensor!'):
    optim.Adam([_param(3)])
  with pytest.raises(NotImplementedError, match='Only support cuda tensor!'):
    optim.Adam([{'params': [_param(3)], 'lr': 1e-2}, {'params': [_param(4, 4)]}], lr=1e-3, betas=(0.8, 0.9), eps=1e-6, weight_decay=0.1,
               skip_nonfinite=False, max_grad_norm=1.0)
  with pytest.raises(TypeError, match='fp32'):
    optim.Adam([_param(3, dtype=torch.float64)])
  with pytest.raises(TypeError, match='fp32'):
    optim.Adam([_param(3), _param(3, dtype=torch.bfloat16)])
  with pytest.raises(ValueError, match='contiguous'):
    optim.Adam([torch.nn.Parameter(torch.zeros(3, 4).t())])
  with pytest.raises(ValueError, match='one device'):
    optim.Adam([_param(3), _param(3, device='meta')])
  frozen = _param(3)
  frozen.requires_grad_(False)
  with pytest.raises(ValueError, match='no parameter requires a gradient'):  # parameters that take no gradient are left out: none is left
    optim.Adam([frozen])
  with pytest.raises(NotImplementedError):  # ... and a frozen one of another dtype does not count
    frozen64 = _param(3, dtype=torch.float64)
    frozen64.requires_grad_(False)
    optim.Adam([frozen64, _param(3)])
  for bad in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(weight_decay=-1.0)):  # torch's own argument checks
    with pytest.raises(ValueError, match='Invalid'):
      optim.Adam([_param(3)], **bad)


def test_the_entries_refuse_bad_arguments_before_any_launch():
  lib = mode_hip.lib()
  null, one, odd = ctypes.c_void_p(0), ctypes.c_void_p(64), ctypes.c_void_p(68)
  big = 1 << 20
  ok_prepare = [one, 100, one, big, one, 2, 1, null]
  for at, bad, code, msg in [(0, null, -1, b'null pointer'), (4, null, -1, b'null pointer'), (1, 0, -1, b'bad sizes'), (1, -5, -1, b'bad sizes'),
                             (5, 0, -1, b'bad sizes'), (4, odd, -1, b'misaligned'), (2, null, -3, b'workspace'), (2, odd, -3, b'workspace'),
                             (3, 8, -3, b'too small')]:
    args = list(ok_prepare)
    args[at] = bad
    assert lib.mode_adam_prepare(*args) == code and msg in lib.mode_last_error(), (at, bad, lib.mode_last_error())
  ok_update = [one, 7, one, 11, one, one, one, one, 2, null]
  for at, bad, msg in [(0, null, b'table missing'), (2, null, b'table missing'), (4, null, b'null pointer'), (5, null, b'null pointer'),
                       (6, null, b'null pointer'), (7, null, b'null pointer'), (1, 0, b'bad sizes'), (3, 0, b'bad sizes'), (3, -1, b'bad sizes'),
                       (8, 0, b'bad sizes'), (7, odd, b'misaligned'), (0, odd, b'misaligned')]:
    args = list(ok_update)
    args[at] = bad
    assert lib.mode_adam_update(*args) == -1 and msg in lib.mode_last_error(), (at, bad, lib.mode_last_error())
  # the two size queries launch nothing and say what the Python side allocates
  assert lib.mode_adam_workspace_bytes(0) == 0 and lib.mode_adam_workspace_bytes(1) == 16
  assert lib.mode_adam_workspace_bytes(sum(SIZES)) == 16 * -(-sum(SIZES) // 1024)  # one (sum, count) column per block of 256 quads
  assert lib.mode_adam_workspace_bytes(1 << 40) == 16 * 1024  # the grid is capped
  assert lib.mode_adam_block_bytes(0) == 0 and lib.mode_adam_block_bytes(2) == 8 * (8 + 16) + 4 * (8 + 16)


def test_the_new_entries_are_named_for_what_they_do():
  """mode_hip.LAUNCHING holds the entries with a stream parameter: the two that launch are in it and take the stream last, the two size
  queries are not."""
  names = sorted(n for n in mode_hip.SIGNATURES if n.startswith('mode_adam_'))
  assert names == ['mode_adam_block_bytes', 'mode_adam_prepare', 'mode_adam_update', 'mode_adam_workspace_bytes']
  for n in ('mode_adam_prepare', 'mode_adam_update'):
    assert n in mode_hip.LAUNCHING and mode_hip.SIGNATURES[n][1][-1] is ctypes.c_void_p
  for n in ('mode_adam_block_bytes', 'mode_adam_workspace_bytes'):
    assert n not in mode_hip.LAUNCHING
  assert optim.SEGMENT.itemsize == 32 and optim.CHUNK_RECORD.itemsize == 16 and optim.CHUNK == 2048  # the header's records


@pytest.mark.parametrize('sizes,groups', [(SIZES, GROUPS), ([1], [0]), ([4096 * 3], [0]), ([2048, 2049, 2047, 1], [1, 0, 2, 0])])
def test_chunk_table(sizes, groups):
  seg, ch = optim.build_tables(sizes, groups, addresses=[4096 * (i + 1) for i in range(len(sizes))])
  n = sum(sizes)
  assert seg['numel'].tolist() == sizes and seg['group'].tolist() == groups
  assert seg['first'].tolist() == [sum(sizes[:i]) for i in range(len(sizes))]
  assert seg['param'].tolist() == [4096 * (i + 1) for i in range(len(sizes))]
  covered = np.zeros(n, dtype=np.int64)
  for off, s, count in ch.tolist():
    assert 1 <= count <= optim.CHUNK
    assert seg['first'][s] <= off and off + count <= seg['first'][s] + seg['numel'][s], 'a chunk crosses its segment'
    assert (off - seg['first'][s]) % optim.CHUNK == 0  # chunks start at multiples of the chunk size inside their tensor
    covered[off:off + count] += 1
  assert (covered == 1).all(), 'every element exactly once'
  assert len(ch) == sum(-(-k // optim.CHUNK) for k in sizes)
  assert [groups[s] for s in ch['seg'].tolist()] == [g for k, g in zip(sizes, groups) for _ in range(-(-k // optim.CHUNK))]
  assert ch['off'].tolist() == sorted(ch['off'].tolist())  # in flat order
  if sizes == SIZES:  # the two long tensors: two whole chunks and a tail of 1 and of 2 elements
    assert [c for _, s, c in ch.tolist() if s == 4] == [2048, 2048, 1] and [c for _, s, c in ch.tolist() if s == 5] == [2048, 2048, 2]


def test_chunk_table_refusals():
  with pytest.raises(ValueError):
    optim.build_tables([], [])
  with pytest.raises(ValueError):
    optim.build_tables([3, 0], [0, 0])
  with pytest.raises(ValueError):
    optim.build_tables([3, 4], [0])
