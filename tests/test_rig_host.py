"""Camera rigs, CPU tier: the rig tables and their validation, the host-side argument checks of the four mode_multiview_rig_handoff
entries (no launch), the module contract of ModeMultiView(rig=) and the ingest's slot table."""
import copy
import ctypes
import json
import math
import os
import pickle

import numpy as np
import pytest
import torch

import mode_hip
import models
from dataloader import gpu_ingest
from models import mode_multiview
from utils import geometry as HG
from utils import rig as RG
from utils.rig import CameraRig, PairPose

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ENTRIES = ('mode_multiview_rig_handoff_workspace_bytes', 'mode_multiview_rig_handoff', 'mode_multiview_rig_handoff_bwd',
           'mode_multiview_rig_handoff_bwd_full')


# ------------------------------------------------------------------------------------------------ the rig as data
def test_deep360_is_the_geometry_tables_bit_for_bit():
  r = CameraRig.deep360()
  assert r.names == HG.PAIRS and r.rgb == (0, 1, 10, 11) == mode_multiview.FUSION_RGB and len(r) == 6
  base = HG._baselines('Deep360')
  for k, p in enumerate(r.pairs):
    assert np.float32(p.baseline).tobytes() == base[k].tobytes() and isinstance(p.baseline, float)
    if p.name in HG._ROT_PITCH:
      assert p.kind == 'rotate' and p.pose == (HG._ROT_PITCH[p.name], 0, 0)
    elif p.name in HG._VIEW_POSES:
      assert p.kind == 'view' and p.pose == tuple(HG._VIEW_POSES[p.name])
    else:
      assert p.name == '12' and p.kind == 'identity' and p.pose == ()
  rec, R, V = r.records()
  assert (R, V) == (2, 3) and rec.dtype.itemsize == 12
  assert rec['kind'].tolist() == [0, 1, 1, 2, 2, 2] and rec['table'].tolist() == [0, 0, 1, 0, 1, 2]
  assert rec['baseline'].tobytes() == base.tobytes()
  assert r.deep360_layout and not r.subset(('12', '13', '23')).deep360_layout


def test_square():
  d, one, half = CameraRig.deep360(), CameraRig.square(1.0), CameraRig.square(0.5)
  assert one == d and hash(one) == hash(d) and not (one != d)
  assert [(p.name, p.baseline, p.kind, p.pose) for p in one.pairs] == [(p.name, p.baseline, p.kind, p.pose) for p in d.pairs]
  assert half != d and half.rgb == d.rgb
  for a, b in zip(half.pairs, d.pairs):
    assert a.name == b.name and a.kind == b.kind and a.baseline == 0.5 * b.baseline
    if a.kind == 'view':
      assert a.pose[:3] == tuple(0.5 * v for v in b.pose[:3]) and a.pose[3:] == b.pose[3:]
    else:
      assert a.pose == b.pose
  s = CameraRig.square(0.6 * math.sqrt(2))  # the consistent counterpart of dbname='other': its baselines, to the last float32 bit
  assert np.abs(np.array([p.baseline for p in s.pairs], dtype=np.float32).view(np.int32) - HG._baselines('other').view(np.int32)).max() <= 1
  assert [p.baseline for p in s.pairs[:2]] == [float(b) for b in HG._baselines('other')[:2]]
  assert s.pairs[4].pose[1] == -0.6 * math.sqrt(2) and HG._VIEW_POSES['24'][1] == -1  # where 'other' keeps the unit square
  for bad in (0.0, -1.0, float('nan'), float('inf')):
    with pytest.raises(ValueError, match='side'):
      CameraRig.square(bad)


def test_subset():
  d = CameraRig.deep360()
  s = d.subset(('23', '12', '34'))
  assert s.names == ('23', '12', '34') and s.pairs == (d.pairs[3], d.pairs[0], d.pairs[5])
  assert s.rgb == (2, 3, 4, 5)  # panoramas 0, 1 of pair 12 (now pair 1) and 10, 11 of pair 34 (now pair 2), in the parent's order
  assert d.subset(('12', '13', '23')).rgb == (0, 1) and d.subset(('34',)).rgb == (0, 1)
  assert d.subset(('13', '12'), rgb=(3, 0)).rgb == (3, 0)
  assert d.subset(HG.PAIRS) == d
  with pytest.raises(ValueError, match="RGB.*13, 14"):
    d.subset(('13', '14'))
  assert d.subset(('13', '14'), rgb=(0,)).rgb == (0,)
  with pytest.raises(ValueError, match="no pair '15'"):
    d.subset(('12', '15'))
  with pytest.raises(ValueError, match="'12' appears twice"):
    d.subset(('12', '12'))
  rec, R, V = d.subset(('34', '14', '12', '23')).records()
  assert (R, V) == (1, 2) and rec['kind'].tolist() == [2, 1, 0, 2] and rec['table'].tolist() == [0, 0, 0, 1]


def test_validation_names_the_pair():
  ok = PairPose('a', 1.0, 'identity')
  cases = [
      (lambda: PairPose('p1', 0.0, 'identity'), "'p1'.*baseline"),
      (lambda: PairPose('p2', -1.0, 'identity'), "'p2'.*baseline"),
      (lambda: PairPose('p3', float('nan'), 'identity'), "'p3'.*baseline"),
      (lambda: PairPose('p4', float('inf'), 'identity'), "'p4'.*baseline"),
      (lambda: PairPose('p5', 1e-50, 'identity'), "'p5'.*baseline"),  # 0 in float32
      (lambda: PairPose('p6', 'x', 'identity'), "'p6'.*numbers"),
      (lambda: PairPose('p7', 1.0, 'shear'), "'p7'.*kind"),
      (lambda: PairPose('p8', 1.0, 'identity', (0.1,)), "'p8'.*0 numbers, got 1"),
      (lambda: PairPose('p9', 1.0, 'rotate', (0.1, 0.2)), "'p9'.*3 numbers, got 2"),
      (lambda: PairPose('p10', 1.0, 'view', (0, 0, 0)), "'p10'.*6 numbers, got 3"),
      (lambda: PairPose('p11', 1.0, 'rotate', (0.1, float('nan'), 0)), "'p11'.*finite"),
      (lambda: PairPose('p12', 1.0, 'view', (0, float('inf'), 0, 0, 0, 0)), "'p12'.*finite"),
      (lambda: CameraRig([ok, PairPose('a', 2.0, 'identity')], (0,)), "'a' appears twice"),
      (lambda: CameraRig([], (0,)), '0 pairs'),
      (lambda: CameraRig([PairPose(str(k), 1.0, 'identity') for k in range(17)], (0,)), '17 pairs'),
      (lambda: CameraRig([ok], (2,)), r'rgb panorama 2 is outside \[0, 2\).*\(a\)'),
      (lambda: CameraRig([ok], (-1,)), 'rgb panorama -1'),
      (lambda: CameraRig([ok], (0, 0)), 'twice'),
      (lambda: CameraRig([ok, 'b'], (0,)), 'pair 1 is'),
      (lambda: CameraRig([ok], 3), 'rgb must be a sequence'),
      (lambda: CameraRig([ok], ()), 'rgb is empty'),
  ]
  for make, text in cases:
    with pytest.raises(ValueError, match=text):
      make()
  assert RG.MAX_PAIRS == 16 and len(CameraRig([PairPose(str(k), 1.0, 'identity') for k in range(16)], (31,))) == 16


def test_hashing_and_equality():
  a = PairPose('x', 0.26, 'rotate', (math.pi / 3, 0.2, -0.1))
  b = PairPose('x', np.float32(0.26), 'rotate', [math.pi / 3, 0.2, -0.1])
  assert a == b and hash(a) == hash(b) and a.baseline == float(np.float32(0.26))
  assert a != PairPose('x', 0.26, 'rotate', (math.pi / 3, 0.2, 0.1)) and a != PairPose('y', 0.26, 'rotate', a.pose) and a != 'x'
  r1, r2 = CameraRig([a], (0,)), CameraRig((b,), [0], name='another label')
  assert r1 == r2 and hash(r1) == hash(r2) and {r1: 1}[r2] == 1
  assert r1 != CameraRig([a], (1,)) and r1 != CameraRig([a], (0, 1))
  d = CameraRig.deep360()
  assert CameraRig(reversed(d.pairs), d.rgb) != d
  assert len({d, CameraRig.square(1.0), CameraRig.square(0.5), d.subset(('12',))}) == 3
  with pytest.raises(AttributeError):
    a.baseline = 2.0
  with pytest.raises(AttributeError):
    d.rgb = (0,)
  # the docstring a user fills the poses in from states both conventions
  doc = PairPose.__doc__
  assert '(pitch, yaw, roll)' in doc and '(y0, z0, x0, pitch, yaw, roll)' in doc and 'Rx(roll) Rz(yaw) Ry(pitch)' in doc and 'R (X1 - t)' in doc
  assert "dbname='other'" in CameraRig.square.__doc__


def test_copy_and_pickle_round_trip():
  """Immutable with __slots__: copies and pickles rebuild through the constructor, so a module that holds a rig can be deep-copied
  (EMA / AveragedModel), saved whole and sent to loader workers."""
  pose = PairPose('x', 0.26, 'view', (0.3, -0.5, 0.4, 1.0, 0.2, -0.3))
  rigs = (CameraRig.deep360(), CameraRig.square(0.5).subset(('23', '12'), rgb=(3,)), CameraRig([pose], (1, 0), name='one'))
  for obj in (pose,) + rigs:
    for twin in (copy.copy(obj), copy.deepcopy(obj), pickle.loads(pickle.dumps(obj)), pickle.loads(pickle.dumps(obj, protocol=2))):
      assert type(twin) is type(obj) and twin == obj and hash(twin) == hash(obj) and repr(twin) == repr(obj)
  for rig in rigs:
    twin = pickle.loads(pickle.dumps(rig))
    assert twin.name == rig.name and twin.pairs == rig.pairs and twin.rgb == rig.rgb and {rig: 1}[twin] == 1
    rec, want = twin.records(), rig.records()
    assert rec[0].tobytes() == want[0].tobytes() and rec[1:] == want[1:]
  rig = rigs[1]
  net = models.ModeMultiView(16, 10., 64, 32, channels=(8, 16, 32, 64), rig=rig)
  twin = copy.deepcopy(net)
  assert twin.rig == rig and twin.rig is not None and twin.pairs == 2
  assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), twin.state_dict().values()))
  assert copy.deepcopy(models.ModeMultiView(16, 10., 64, 32, channels=(8, 16, 32, 64))).rig is None


# ------------------------------------------------------------------------------------------------ the C entries, without a launch
def test_the_four_entries_and_their_names():
  for n in ENTRIES:
    assert n in mode_hip.SIGNATURES and hasattr(mode_hip.lib(), n)
  assert ENTRIES[0] not in mode_hip.LAUNCHING
  for n in ENTRIES[1:]:
    assert n in mode_hip.LAUNCHING and mode_hip.SIGNATURES[n][1][-1] is ctypes.c_void_p  # the stream is the last argument
  with open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'mode_hip.h')) as f:
    header = f.read()
  for n in ENTRIES:
    assert n + '(' in header
  assert RG.MAX_PAIRS == mode_hip.CONSTANTS['MODE_MV_MAX_PAIRS'] == 16  # utils.rig imports no binding: its two restated values are held to the header here
  assert RG.PAIR_RECORD == np.dtype(mode_hip._header.structure(mode_hip.HEADER, 'mode_mv_pair'))
  assert mode_hip.HEADER.records['mode_mv_pair'] == [('kind', 'int32_t', None), ('table', 'int32_t', None), ('baseline', 'float', None)]
  assert mode_hip.lib().mode_hip_abi_version() == 31  # additive: tests/test_abi.py pins the number


def _records(kinds, tables=None, baselines=None):
  rec = np.zeros(len(kinds), dtype=RG.PAIR_RECORD)
  count = [0, 0, 0]
  for i, k in enumerate(kinds):
    rec[i] = (k, count[k % 3] if tables is None else tables[i], 1.0 if baselines is None else baselines[i])
    count[k % 3] += 1
  return rec


def test_rig_entries_validate_on_the_host():
  lib = mode_hip.lib()
  q = lib.mode_multiview_rig_handoff_workspace_bytes
  assert q(2, 3, 64, 32) == 8 * 3 * 2 * 64 * 32 and q(5, 16, 40, 24) == 8 * 16 * 5 * 40 * 24 and q(1, 1, 1, 1) == 8
  assert q(2, 0, 64, 32) == 0 and q(0, 3, 64, 32) == 0
  big = 2 ** 31 - 1  # sizes whose products pass 2^63: 0, as for every size the launching entries refuse
  assert q(big, 16, big, big) == 0 and q(1, 1, big, big) == 0 and q(big, 1, 1, 1) == 0 and q(1, 1, 1 << 15, 1 << 15) == 0
  assert q(1, 1, 1 << 15, (1 << 15) - 1) == 8 * (1 << 15) * ((1 << 15) - 1) and q(2, 1, 1 << 15, (1 << 15) - 1) == 0
  assert q(1, -1, 64, 32) == 0 and q(1, 3, -1, 32) == 0 and q(1, 3, 64, 0) == 0 and q(-1, 3, 64, 32) == 0 and q(1, 17, 64, 32) == 0
  null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
  xf = (ctypes.c_double * (12 * 16))()
  xfp = ctypes.cast(xf, ctypes.c_void_p)
  mixed = _records([0, 1, 1, 2, 2, 2])

  def fwd(F=1, H=64, W=32, rec=mixed, P=None, R=2, V=3, disp=one, conf=one, grids=one, trig=one, x=xfp, flags=0, out=one, ws=one, pairs=None):
    pp = ctypes.c_void_p(rec.ctypes.data) if pairs is None else pairs
    return lib.mode_multiview_rig_handoff(disp, conf, F, len(rec) if P is None else P, H, W, pp, R, grids, trig, V, x, flags, out, ws, null)

  def bwd(full, F=1, H=64, W=32, rec=mixed, P=None, R=2, V=3, disp=one, gout=one, keys=one, trig=one, x=xfp, rowptr=one, target=one,
          weight=one, n_adj=8, flags=0, gdisp=one, gconf=one, pairs=None):
    pp = ctypes.c_void_p(rec.ctypes.data) if pairs is None else pairs
    head = (disp, gout, keys, F, len(rec) if P is None else P, H, W, pp, R, trig, V, x, rowptr, target, weight, n_adj, flags, gdisp)
    if full:
      return lib.mode_multiview_rig_handoff_bwd_full(*(head + (gconf, null)))
    return lib.mode_multiview_rig_handoff_bwd(*(head + (null,)))

  err = lib.mode_last_error
  for call in (fwd, lambda **kw: bwd(False, **kw), lambda **kw: bwd(True, **kw)):
    # P
    assert call(P=0) == -1 and b'pairs' in err()
    assert call(P=17) == -1 and b'pairs' in err()
    assert call(P=-3) == -1
    # sizes: H, W <= 0, F < 0, element counts >= 2^31
    assert call(F=-1) == -1 and b'bad size' in err()
    assert call(H=0) == -1 and call(W=-4) == -1
    assert call(F=1 << 9, H=1024, W=1024) == -1 and b'bad size' in err()  # 2 P F H W = 12 * 2^29
    assert call(F=1 << 8, H=1024, W=1024, rec=_records([0] * 16), R=0, V=0) == -1 and b'bad size' in err()  # 32 * 2^28
    big = 2 ** 31 - 1  # products beyond 2^63 are refused like any other size, not formed
    assert call(F=big, H=big, W=big) == -1 and b'bad size' in err()
    assert call(F=1, H=big, W=big) == -1 and b'bad size' in err()
    assert call(F=big, H=1, W=1, rec=_records([0]), R=0, V=0) == -1 and b'bad size' in err()  # 2 F = 2^32 - 2
    assert call(F=0, H=1 << 16, W=1 << 15) == -1 and call(F=0, H=1 << 16, W=(1 << 15) - 1) == 0  # H W < 2^31 whatever F is
    assert call(flags=4) == -1 and b'flags' in err()
    # the records
    assert call(pairs=null) == -1 and b'null pointer' in err()
    assert call(rec=_records([0, 3, 1, 2, 2, 2])) == -1 and b'pair 1 has unknown kind 3' in err()
    assert call(rec=_records([0, -1, 1, 2, 2, 2])) == -1 and b'unknown kind' in err()
    assert call(R=1) == -1 and call(R=3) == -1 and call(V=2) == -1 and call(V=4) == -1 and call(R=-1) == -1 and call(V=-1) == -1
    assert call(R=3, V=2) == -1
    assert call(rec=_records([0, 0, 0]), R=1, V=0) == -1 and b'0 rotations' in err()
    assert call(rec=_records([0, 0, 0]), R=0, V=1) == -1 and b'0 view transforms' in err()
    assert call(rec=_records([0, 1, 1, 2, 2, 2], tables=[0, 0, 2, 0, 1, 2])) == -1 and b'pair 2 has table index 2' in err()
    assert call(rec=_records([0, 1, 1, 2, 2, 2], tables=[0, 0, 1, 0, 1, 3])) == -1 and b'pair 5 has table index 3' in err()
    assert call(rec=_records([0, 1, 1, 2, 2, 2], tables=[0, 0, -1, 0, 1, 2])) == -1 and b'table index -1' in err()
    assert call(rec=_records([0, 1, 1, 2, 2, 2], tables=[0, 0, 0, 0, 1, 2])) == -1 and b'second time' in err()
    assert call(rec=_records([0, 1, 1, 2, 2, 2], tables=[0, 0, 1, 0, 1, 1])) == -1 and b'second time' in err()
    assert call(F=0, rec=_records([0, 1, 1, 2, 2, 2], tables=[9, 1, 0, 2, 0, 1])) == 0  # any permutation; an identity pair's index is ignored
    assert call(x=null) == -1 and b'null pointer' in err()
    assert call(disp=null) == -1 and b'null pointer' in err()
    assert call(trig=null) == -1 and b'null pointer' in err()
    # F = 0 is a no-op, whatever the device pointers are
    kw = dict(F=0, disp=null, trig=null)
    assert call(**kw) == 0

  for kwd in ('conf', 'grids', 'out'):
    assert fwd(**{kwd: null}) == -1 and b'null pointer' in err(), kwd
  assert fwd(grids=ctypes.c_void_p(20)) == -1 and b'aligned' in err()
  assert fwd(ws=null) == -3 and b'workspace' in err()
  assert fwd(ws=ctypes.c_void_p(20)) == -3 and b'workspace' in err()
  assert fwd(F=0, disp=null, conf=null, out=null, ws=null, grids=null, trig=null) == 0
  for full in (False, True):
    for kwd in ('gout', 'rowptr', 'gdisp', 'target', 'weight'):
      assert bwd(full, **{kwd: null}) == -1 and b'null pointer' in err(), kwd
    assert bwd(full, n_adj=-1) == -1 and bwd(full, n_adj=4 * 2 * 64 * 32 + 1) == -1 and b'adjoint' in err()
    assert bwd(full, keys=null) == -3 and b'key planes' in err()
    assert bwd(full, keys=ctypes.c_void_p(20)) == -3 and b'key planes' in err()
    assert bwd(full, F=0, disp=null, gout=null, keys=null, gdisp=null, gconf=null, rowptr=null, target=null, weight=null) == 0
  assert bwd(True, gconf=null) == -1 and b'null pointer' in err()
  assert bwd(True, flags=2) == -1 and b'no confidence channels' in err()
  assert bwd(True, flags=1) == -1 and b'no gradient' in err()


# ------------------------------------------------------------------------------------------------ the module
def _manifest(name):
  with open(os.path.join(GOLDEN, name)) as f:
    return [(k, tuple(s)) for k, s in json.load(f)]


def _tiny(**kw):
  return models.ModeMultiView(16, 10., 64, 32, channels=(8, 16, 32, 64), **kw)


def test_without_a_rig_the_state_dict_is_what_it_was():
  """(Passes before and after this feature.)"""
  net = models.ModeMultiView(16, 10., 64, 32)
  want = [('disparity.' + k, s) for k, s in _manifest('manifest_mode_disparity.json')] + [('fusion.' + k, s) for k, s in _manifest('manifest_mode_fusion.json')]
  assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == want


def test_module_contract_with_a_rig():
  d = CameraRig.deep360()
  plain, full = _tiny(), _tiny(rig=d)
  assert [(k, v.shape) for k, v in full.state_dict().items()] == [(k, v.shape) for k, v in plain.state_dict().items()]
  assert full.rig == d and full.pairs == 6 and plain.rig is None and plain.pairs == 6
  for names, k in ((('12', '13', '23'), 2), (('12', '34', '14'), 4)):
    net = _tiny(rig=d.subset(names))
    fe = net.fusion.feature_extraction
    w_d, w_r = next(iter(fe.depth_layer1.parameters())), next(iter(fe.rgb_layer1.parameters()))
    assert tuple(w_d.shape) == (8, 6, 3, 3) and tuple(w_r.shape) == (8, 3 * k, 3, 3)
    other = {key: tuple(v.shape) for key, v in net.state_dict().items()}
    ref = {key: tuple(v.shape) for key, v in plain.state_dict().items()}
    differ = sorted(key for key in ref if ref[key] != other[key])
    first = ['fusion.feature_extraction.depth_layer1.0.conv1.0.0.weight', 'fusion.feature_extraction.rgb_layer1.0.conv1.0.0.weight']
    assert list(other) == list(ref) and differ == first[:1 if k == 4 else 2]  # (four RGB panoramas are Deep360's twelve planes)
  big = models.ModeMultiView(16, 10., 64, 32, rig=d.subset(('12', '13', '23')))
  assert tuple(next(iter(big.fusion.feature_extraction.depth_layer1.parameters())).shape) == (32, 6, 3, 3)
  assert tuple(next(iter(big.fusion.feature_extraction.rgb_layer1.parameters())).shape) == (32, 6, 3, 3)
  one = _tiny(rig=CameraRig([PairPose('v', 0.26, 'view', (0.3, -0.5, 0.4, 1.0, 0.2, -0.3))], (0,)))
  assert tuple(next(iter(one.fusion.feature_extraction.depth_layer1.parameters())).shape) == (8, 2, 3, 3)
  assert tuple(next(iter(one.fusion.feature_extraction.rgb_layer1.parameters())).shape) == (8, 3, 3, 3)


def test_refused_combinations():
  d = CameraRig.deep360()
  three = d.subset(('12', '13', '23'))
  with pytest.raises(ValueError, match='Baseline.*6 pairs'):
    _tiny(rig=three, fusion='Baseline')
  _tiny(rig=d, fusion='Baseline')
  _tiny(rig=CameraRig(reversed(d.pairs), (3,)), fusion='Baseline')
  with pytest.raises(ValueError, match='resize=True.*layout'):
    _tiny(rig=three, resize=True)
  with pytest.raises(ValueError, match='resize=True.*layout'):
    _tiny(rig=d.subset(HG.PAIRS, rgb=(0, 1, 10)), resize=True)
  _tiny(rig=d, resize=True)
  _tiny(rig=CameraRig.square(0.5), resize=True)
  with pytest.raises(ValueError, match='rig= and dbname'):
    _tiny(rig=d, dbname='other')
  with pytest.raises(ValueError, match="handoff_grad"):
    _tiny(rig=three, handoff_grad='full')  # (conf_png=True: as without a rig)
  z = torch.zeros(1, 6, 8, 4)
  with pytest.raises(ValueError, match='rig= and dbname'):
    HG.disp2depth_frames_gpu(z, z, 'other', rig=d)
  with pytest.raises(ValueError, match='rig= and dbname'):
    HG.disp2depth_frames_bwd(z, z, z, 'other', rig=d)
  with pytest.raises(NotImplementedError):  # CPU tensors, as without a rig
    HG.disp2depth_frames_gpu(z[:, :3], z[:, :3], rig=three)
  net = _tiny(rig=three).eval()
  with pytest.raises(NotImplementedError):
    net(torch.zeros(1, 6, 3, 64, 32))
  assert HG._as_frames(torch.zeros(6, 4, 4), 'disp', three).shape == (2, 3, 4, 4)
  assert HG._as_frames(torch.zeros(6, 1, 4, 4), 'disp', three).shape == (2, 3, 4, 4)
  assert HG._as_frames(torch.zeros(2, 3, 4, 4), 'disp', three).shape == (2, 3, 4, 4)
  with pytest.raises(ValueError, match='3 per frame'):
    HG._as_frames(torch.zeros(7, 1, 4, 4), 'disp', three)
  with pytest.raises(ValueError):
    HG._as_frames(torch.zeros(2, 6, 4, 4), 'disp', three)


# ------------------------------------------------------------------------------------------------ the ingest
@pytest.mark.parametrize('want_rgb', [True, False])
@pytest.mark.parametrize('F', [1, 3])
def test_slot_table(F, want_rgb):
  d = CameraRig.deep360()
  assert torch.equal(gpu_ingest._rig_slots(F, d, want_rgb, 'cpu'), gpu_ingest._frame_slots(F, want_rgb, 'cpu'))
  three = d.subset(('23', '12', '13'), rgb=(3, 0, 4))
  slots = gpu_ingest._rig_slots(F, three, want_rgb, 'cpu').numpy()
  assert slots.shape == (6 * F, 2) and slots.dtype == np.int32
  for f in range(F):
    for k in range(6):
      first, second = slots[6 * f + k]
      assert first == (k % 2) * 3 * F + 3 * f + k // 2
      assert second == (6 * F + 3 * f + three.rgb.index(k) if want_rgb and k in three.rgb else -1)
  used = np.concatenate([slots[:, 0], slots[:, 1][slots[:, 1] >= 0]])
  assert sorted(used.tolist()) == list(range((6 + (3 if want_rgb else 0)) * F))  # every slot of the buffer is written, once


def test_split_frames_of_a_rig():
  F, H, W = 2, 2, 4
  three = CameraRig.deep360().subset(('23', '12', '13'), rgb=(3, 0, 4))
  ids = torch.arange(F * 6, dtype=torch.float32).view(F, 6, 1, 1, 1).expand(F, 6, 3, H, W).contiguous()
  left, right, rgb = mode_multiview.split_frames(ids, three)
  assert left.shape == right.shape == (3 * F, 3, H, W) and rgb.shape == (F, 9, H, W)
  for f in range(F):
    for p in range(3):
      assert bool((left[3 * f + p] == 6 * f + 2 * p).all()) and bool((right[3 * f + p] == 6 * f + 2 * p + 1).all())
    for r, pano in enumerate(three.rgb):
      assert bool((rgb[f, 3 * r:3 * r + 3] == 6 * f + pano).all())
  d = CameraRig.deep360()
  full = torch.arange(F * 12 * 3, dtype=torch.float32).view(F, 12, 3, 1, 1).expand(F, 12, 3, H, W).contiguous()
  for a, b in zip(mode_multiview.split_frames(full, d), mode_multiview.split_frames(full)):
    assert torch.equal(a, b)
  with pytest.raises(ValueError, match='3 pairs'):
    mode_multiview.split_frames(full, three)
