"""Time ModeMultiView on whole Deep360 frames (1024 x 512, 192 disparities) and its multi-view hand-off.

    python tools/multiview_bench.py [--frames 1 2 4] [--window 1.0] [--out profiles/multiview_bench.json]
    python tools/multiview_bench.py --once      # one hand-off call and one six-call path at F = 1, for a kernel trace
    python tools/multiview_bench.py --scoring   # the scoring line alone
    python tools/multiview_bench.py --u8        # the ingest line alone: float frames from the host against 8-bit frames, and resize=True
    python tools/multiview_bench.py --train     # the training line alone: fusion_loss + backward per frame, both modes; the hand-off's backward
    python tools/multiview_bench.py --rig       # the rig line alone: the hand-off through the six-pair entries and through the rig entries

For every F: the frame time of the composed module, eager and replayed from a captured graph; the split between stage 1 (ModeDisparity
at batch 6F), the hand-off (utils.geometry.disp2depth_frames_gpu) and stage 2 (the fusion network); and the hand-off against the
six-call path it replaces (six disp2depth_gpu calls per frame + the interleave).  One more line for the scoring stage
(utils.panorama.erp_depth_metrics against the per-frame composition it replaces, F = 1 and 4).  Device events around windows of at least
--window seconds after a warm-up; weights from the test fixtures' recipes, seeded random panoramas (the timings do not depend on the values
beyond the data-dependence of the z-buffer scatter).  Writes one JSON file.

--u8 times one frame from decoded 8-bit panoramas in host memory to the fused depth on the device, three ways, alternating A B C A B C:
  A  host normalisation (dataloader.preprocess on the 12 panoramas) + upload of the float frame (75 MB) + the float forward
  B  upload of the 8-bit frame (19 MB) + the uint8 forward (normalisation and split in one kernel)
  C  upload of the 8-bit frame + the uint8 forward of ModeMultiView(resize=True) (fusion network at half size)
Host clock around work that ends in a device synchronise; medians in ms.

--train times one ModeMultiView.fusion_loss + backward on one frame (F = 1), with stage 1 frozen (net.train(); net.disparity.eval()) and
with stage 1 fine-tuned (net.train(), batch statistics at batch 6), and the hand-off's forward and backward alone on the disparities of
that frame.  Device events around every single call after a warm-up; medians in ms.  One JSON line.  It also carries the figures of
fine-tuning through the confidence (ModeMultiView(handoff_grad='full', conf_png=False)): the head's backward with and without the
confidence gradient at B = 6, D4 = 48, 1024 x 512, timed alternately (head_bwd_ms, head_bwd_conf_ms), the hand-off's backward for both
outputs (handoff_bwd_full_ms) and the 'full' step and its peak memory (fine_tuning_full_step_ms, fine_tuning_full_peak_GiB).

--rig prints the rig line at F = 1: handoff_fwd_ms, handoff_bwd_ms and handoff_bwd_full_ms through the six-pair entries
('six') and through mode_multiview_rig_handoff* with CameraRig.deep360() ('rig_deep360') -- both move the same bytes -- and with its
subset 12, 13, 23 ('rig_subset3'), and the forward of that subset as three single calls ('subset3_single_calls'); the sides of a figure
alternate window by window, a window is about half a second, and beside the device time of every side stands the host time of its calls."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'mode-2022_amd'), os.path.join(ROOT, 'tests', 'golden')):
  if p not in sys.path:
    sys.path.insert(0, p)

import torch  # noqa: E402

import models  # noqa: E402
import numpy as np  # noqa: E402
import recipe  # noqa: E402
from mode_hip import functional as HF  # noqa: E402
from mode_hip.graph_step import GraphedStep  # noqa: E402
from models.mode_multiview import split_frames  # noqa: E402
from utils import evaluation, panorama  # noqa: E402
from utils import geometry as HG  # noqa: E402

DEV = 'cuda:0'
H, W, MAXDISP, MAXDEPTH = 1024, 512, 192, 1000.
PAIRS = ('12', '13', '14', '23', '24', '34')


def timed(fn, window, warmup=3):
  """ms per call of fn over a window of at least `window` seconds (device events), after `warmup` calls."""
  for _ in range(warmup):
    fn()
  torch.cuda.synchronize()
  n = 1
  while True:
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
      fn()
    e.record()
    e.synchronize()
    ms = s.elapsed_time(e)
    if ms >= 1000 * window:
      return ms / n, n
    n = max(n + 1, int(n * 1.25 * 1000 * window / max(ms, 1e-3)))


def six_calls(disp, conf):
  frames = []
  for f in range(disp.shape[0]):
    chans = []
    for p, pair in enumerate(PAIRS):
      chans += list(HG.disp2depth_gpu(disp[f, p], conf[f, p], pair))
    frames.append(torch.stack(chans))
  return torch.stack(frames)


def make_frames(F, seed):
  g = torch.Generator().manual_seed(seed)
  return ((torch.rand(F, 12, 3, H, W, generator=g) - 0.45) / 0.226).to(DEV)


def make_net(resize=False, **kw):
  """The well-conditioned full-size disparity fixture with its running statistics (on unit running statistics the eval forward of
  the recipe weights is not finite) and a recipe fusion state."""
  z = np.load(os.path.join(recipe.HERE, 'model_wc_full.npz'))
  sd = recipe.fixture_state(z)
  sd.update({k[3:]: torch.from_numpy(z[k]).clone() for k in z.files if k.startswith('bn/')})
  net = models.ModeMultiView(MAXDISP, MAXDEPTH, H, W, resize=resize, **kw)
  net.disparity.load_state_dict(sd)
  net.fusion.load_state_dict(recipe.recipe_state(recipe.load_manifest('manifest_mode_fusion.json'), 101))
  return net.to(DEV).eval()


def unfused_scoring(pred, gt, maxdepth=MAXDEPTH):
  """The scoring stage composed from its parts, per frame: cassini2Equirec twice, the aten `<=`, depth_metrics (one copy back each)."""
  rows = []
  for f in range(pred.shape[0]):
    pe, ge = HG.cassini2Equirec(pred[f:f + 1]), HG.cassini2Equirec(gt[f:f + 1].unsqueeze(1))
    rows.append(evaluation.depth_metrics(pe, ge, ge <= maxdepth))
  return np.array(rows)


def scoring_line(reps=50, warmup=5):
  """Fused scoring call against the unfused composition at F = 1 and F = 4, 1024 x 512: alternating A B A B, `reps` repetitions of
  each after a warm-up, device events around every single call (both end in their copy back); medians in ms."""
  row = {'stage': 'scoring', 'size': [H, W], 'reps': reps}
  for F in (1, 4):
    g = torch.Generator().manual_seed(200 + F)
    gt = (torch.rand(F, H, W, generator=g) * 1100).to(DEV)  # about a tenth beyond maxdepth
    pred = (gt.unsqueeze(1) * (1 + 0.1 * torch.randn(F, 1, H, W, generator=g).to(DEV))).contiguous()
    calls = {'fused': lambda: panorama.erp_depth_metrics(pred, gt, MAXDEPTH), 'unfused': lambda: unfused_scoring(pred, gt)}
    assert calls['fused']().tobytes() == calls['unfused']().tobytes()
    for _ in range(warmup):
      for fn in calls.values():
        fn()
    ms = {k: [] for k in calls}
    for _ in range(reps):
      for k, fn in calls.items():
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ms[k].append(s.elapsed_time(e))
    for k in calls:
      row['%s_ms_F%d' % (k, F)] = float(np.median(ms[k]))
    row['speedup_F%d' % F] = row['unfused_ms_F%d' % F] / row['fused_ms_F%d' % F]
  print(json.dumps(row), flush=True)
  return row


def u8_line(reps=20, warmup=3):
  """The ingest line (see the module docstring).  A and B compute the same depth, bit for bit (asserted)."""
  from dataloader import preprocess
  norm = preprocess.get_transform_stage1(augment=False)
  net, half = make_net(), make_net(resize=True)
  frame = np.random.RandomState(300).randint(0, 256, (1, 12, H, W, 3)).astype(np.uint8)  # decoded panoramas, host memory
  frame_t = torch.from_numpy(frame)  # pageable, like the float frame the host transform produces
  parts = {'host_norm': [], 'upload_f32': [], 'forward_f32': [], 'upload_u8': [], 'forward_u8': [], 'forward_u8_resize': []}

  def clock(key, fn):
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    parts[key].append(1e3 * (time.perf_counter() - t0))
    return out

  def a():
    f32 = clock('host_norm', lambda: torch.stack([norm(p) for p in frame[0]]).unsqueeze(0))
    dev = clock('upload_f32', lambda: f32.to(DEV))
    return clock('forward_f32', lambda: net(dev))

  def b():
    dev = clock('upload_u8', lambda: frame_t.to(DEV))
    return clock('forward_u8', lambda: net(dev))

  def c():
    dev = frame_t.to(DEV)
    torch.cuda.synchronize()  # (the upload is B's: only the forward is timed here)
    return clock('forward_u8_resize', lambda: half(dev))

  assert torch.equal(a(), b()) and c().shape == (1, 1, H, W)
  for _ in range(warmup):
    a(), b(), c()
  for v in parts.values():
    del v[:]
  for _ in range(reps):
    a(), b(), c()
  row = {'stage': 'u8_ingest', 'size': [H, W], 'frames': 1, 'reps': reps, 'host_threads': torch.get_num_threads()}
  row.update({k + '_ms': float(np.median(v)) for k, v in parts.items()})
  row['A_host_norm_upload_float_forward_ms'] = float(np.median(np.sum([parts[k] for k in ('host_norm', 'upload_f32', 'forward_f32')], 0)))
  row['B_upload_uint8_forward_ms'] = float(np.median(np.sum([parts[k] for k in ('upload_u8', 'forward_u8')], 0)))
  row['C_upload_uint8_forward_resize_ms'] = float(np.median(np.sum([parts['upload_u8'], parts['forward_u8_resize']], 0)))
  print(json.dumps(row), flush=True)
  return row


def train_line(reps=10, warmup=2):
  """The training line (see the module docstring).  The joint mode is timed last: if the training forward of stage 1 at batch 6 does not
  fit, the line still carries the other figures and the reason."""
  net = make_net()
  frames = make_frames(1, 400)
  gt = (torch.rand(1, H, W, generator=torch.Generator().manual_seed(401)) * 1100).to(DEV)  # about a tenth beyond maxdepth
  row = {'stage': 'train', 'size': [H, W], 'frames': 1, 'reps': reps}

  def each(fn):
    for _ in range(warmup):
      fn()
    ms = []
    for _ in range(reps):
      s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      s.record()
      fn()
      e.record()
      e.synchronize()
      ms.append(s.elapsed_time(e))
    return float(np.median(ms))

  with torch.no_grad():
    left, right, _ = split_frames(frames)
    disp, conf = net.disparity(left, right)
    del left, right
  out, keys = HG.disp2depth_frames_gpu(disp, conf, conf_png=True, return_keys=True)
  gout = torch.randn_like(out)
  row['handoff_fwd_ms'] = each(lambda: HG.disp2depth_frames_gpu(disp, conf, conf_png=True))
  row['handoff_bwd_ms'] = each(lambda: HG.disp2depth_frames_bwd(disp, gout, keys))
  row['handoff_bwd_full_ms'] = each(lambda: HG.disp2depth_frames_bwd(disp, gout, keys, conf_grad=True))
  del out, keys, gout, disp, conf

  # the head's backward at the shape of one frame's six pairs, the two entries in turn (A B A B ...), every call between device events
  size = (MAXDISP, H, W)
  logits = torch.randn(6, 1, MAXDISP // 4, H // 4, W // 4, device=DEV, generator=torch.Generator(DEV).manual_seed(402)) * 3
  gp = torch.randn(6, 1, H, W, device=DEV, generator=torch.Generator(DEV).manual_seed(403))
  gc = torch.randn(6, 1, H, W, device=DEV, generator=torch.Generator(DEV).manual_seed(404))
  pred, cf = HF.head_fwd(logits, size, with_confidence=True)
  pair = {'head_bwd_ms': lambda: HF.head_bwd(logits, gp, size), 'head_bwd_conf_ms': lambda: HF.head_bwd_conf(logits, pred, cf, gp, gc, size)}
  ms = {k: [] for k in pair}
  for i in range(warmup + 2 * reps):
    for k, fn in pair.items():
      s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      s.record()
      fn()
      e.record()
      e.synchronize()
      if i >= warmup:
        ms[k].append(s.elapsed_time(e))
  row.update({k: float(np.median(v)) for k, v in ms.items()})
  row['head_bwd_conf_over_head_bwd'] = row['head_bwd_conf_ms'] / row['head_bwd_ms']
  del logits, gp, gc, pred, cf

  def step():
    net.zero_grad(set_to_none=True)
    loss, _ = net.fusion_loss(frames, gt)
    loss.backward()
    return loss

  net.train()
  net.disparity.eval()
  row['frozen_stage1_step_ms'] = each(step)
  row['frozen_stage1_loss'] = float(step().detach())
  net.train()
  try:
    row['fine_tuning_step_ms'] = each(step)
    row['fine_tuning_loss'] = float(step().detach())
    row['fine_tuning_peak_GiB'] = torch.cuda.max_memory_allocated() / 2.0 ** 30
  except torch.cuda.OutOfMemoryError as e:
    row['fine_tuning_step_ms'] = None
    row['fine_tuning_error'] = str(e).splitlines()[0]
  # the same step through the confidence as well: one head pass for both outputs, the hand-off's backward for both
  del net
  torch.cuda.empty_cache()
  net = make_net(conf_png=False, handoff_grad='full')
  net.train()
  torch.cuda.reset_peak_memory_stats()
  try:
    row['fine_tuning_full_step_ms'] = each(step)
    row['fine_tuning_full_loss'] = float(step().detach())
    row['fine_tuning_full_peak_GiB'] = torch.cuda.max_memory_allocated() / 2.0 ** 30
  except torch.cuda.OutOfMemoryError as e:
    row['fine_tuning_full_step_ms'] = None
    row['fine_tuning_full_error'] = str(e).splitlines()[0]
  print(json.dumps(row), flush=True)
  return row


def rig_line(calls=None, windows=4, warmup=20):
  """The hand-off on a rig description (see the module docstring): at F = 1, 1024 x 512, per side the time per call over `windows`
  windows of `calls` calls each (default: 4000 for the forward, 1500 for the gradients -- windows of about half a second, so that the
  clock's ramp and the scheduler are a small part of one).  The sides of a group alternate window by window (A B A B ..., as
  tools/optim_bench.py takes them), so that a drift of the clocks falls on all of them alike.  Per window two times: the device's, from
  two events around the window, and the host's, from a host clock around the un-synchronised calls (the device is idle when a window
  starts).  A call is two torch.empty and one ctypes call; where the host's time per call is not clearly below the device's, the device
  figure is set by the enqueue rate and not by the kernels.  Every figure is [median, min, max] over its windows."""
  from utils.rig import CameraRig
  full = CameraRig.deep360()
  sub = full.subset(('12', '13', '23'))
  idx = [full.names.index(n) for n in sub.names]
  g = torch.Generator().manual_seed(500)
  disp = (torch.rand(1, 6, H, W, generator=g) * 40).to(DEV)
  conf = torch.rand(1, 6, H, W, generator=g).to(DEV)
  gout = torch.randn(1, 12, H, W, generator=g).to(DEV)
  d3, c3 = disp[:, idx].contiguous(), conf[:, idx].contiguous()
  g3 = gout[:, [c for p in idx for c in (2 * p, 2 * p + 1)]].contiguous()
  keys = HG.disp2depth_frames_gpu(disp, conf, conf_png=True, return_keys=True)[1]
  keys3 = HG.disp2depth_frames_gpu(d3, c3, rig=sub, conf_png=True, return_keys=True)[1]
  assert torch.equal(HG.disp2depth_frames_gpu(disp, conf, rig=full, conf_png=True), HG.disp2depth_frames_gpu(disp, conf, conf_png=True))

  def singles():  # the P single-call path of the subset
    return [HG.disp2depth_gpu(d3[0, p], c3[0, p], n) for p, n in enumerate(sub.names)]

  groups = {
      'handoff_fwd_ms': {'six': lambda: HG.disp2depth_frames_gpu(disp, conf, conf_png=True),
                         'rig_deep360': lambda: HG.disp2depth_frames_gpu(disp, conf, rig=full, conf_png=True),
                         'rig_subset3': lambda: HG.disp2depth_frames_gpu(d3, c3, rig=sub, conf_png=True),
                         'subset3_single_calls': singles},
      'handoff_bwd_ms': {'six': lambda: HG.disp2depth_frames_bwd(disp, gout, keys),
                         'rig_deep360': lambda: HG.disp2depth_frames_bwd(disp, gout, keys, rig=full),
                         'rig_subset3': lambda: HG.disp2depth_frames_bwd(d3, g3, keys3, rig=sub)},
      'handoff_bwd_full_ms': {'six': lambda: HG.disp2depth_frames_bwd(disp, gout, keys, conf_grad=True),
                              'rig_deep360': lambda: HG.disp2depth_frames_bwd(disp, gout, keys, rig=full, conf_grad=True),
                              'rig_subset3': lambda: HG.disp2depth_frames_bwd(d3, g3, keys3, rig=sub, conf_grad=True)},
  }
  row = {'stage': 'rig', 'size': [H, W], 'frames': 1, 'windows': windows, 'calls_per_window': {},
         'figures': '[median, min, max] ms per call: <name> device time, <name>_host host time of the un-synchronised calls'}
  per_window = calls
  for name, sides in groups.items():
    calls = per_window or (4000 if name == 'handoff_fwd_ms' else 1500)
    row['calls_per_window'][name] = calls
    ms, host = {k: [] for k in sides}, {k: [] for k in sides}
    for fn in sides.values():
      for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    for _ in range(windows):
      for k, fn in sides.items():
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        s.record()
        for _ in range(calls):
          fn()
        e.record()
        host[k].append(1e3 * (time.perf_counter() - t0) / calls)
        e.synchronize()
        ms[k].append(s.elapsed_time(e) / calls)
    row[name] = {k: [float(np.median(v)), float(min(v)), float(max(v))] for k, v in ms.items()}
    row[name + '_host'] = {k: [float(np.median(v)), float(min(v)), float(max(v))] for k, v in host.items()}
  print(json.dumps(row), flush=True)
  return row


def once():
  disp = (torch.rand(1, 6, H, W, device=DEV) * 40).contiguous()
  conf = torch.rand(1, 6, H, W, device=DEV)
  HG.disp2depth_frames_gpu(disp, conf, conf_png=True)
  torch.cuda.synchronize()
  six_calls(disp.view(1, 6, H, W), conf.view(1, 6, H, W))
  torch.cuda.synchronize()
  print('once: one hand-off call and one six-call path at F = 1, 1024 x 512')


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--frames', type=int, nargs='+', default=[1, 2, 4])
  ap.add_argument('--window', type=float, default=1.0)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'multiview_bench.json'))
  ap.add_argument('--once', action='store_true')
  ap.add_argument('--scoring', action='store_true', help='only the scoring line')
  ap.add_argument('--u8', action='store_true', help='only the ingest line: float frames from the host against 8-bit frames, and resize=True')
  ap.add_argument('--train', action='store_true', help='only the training line: fusion_loss + backward in both modes, the hand-off\'s backward')
  ap.add_argument('--rig', action='store_true', help='only the rig line: the hand-off through the six-pair entries and through the rig entries')
  ap.add_argument('--calls', type=int, default=None, help='--rig: calls per window (default 4000 for the forward, 1500 for the gradients)')
  args = ap.parse_args()
  if args.once:
    return once()
  if args.rig:
    return rig_line(calls=args.calls)
  if args.scoring:
    return scoring_line()
  if args.u8:
    return u8_line()
  if args.train:
    return train_line()
  net = make_net()
  rows = []
  for F in args.frames:
    t0 = time.time()
    frames = make_frames(F, 100 + F)
    with torch.no_grad():
      left, right, rgb = split_frames(frames)
      disp, conf = net.disparity(left, right)
      fi = HG.disp2depth_frames_gpu(disp, conf, conf_png=True)
      ms_eager, n_eager = timed(lambda: net(frames), args.window)
      ms_s1, _ = timed(lambda: net.disparity(left, right), args.window)
      ms_ho, _ = timed(lambda: HG.disp2depth_frames_gpu(disp, conf, conf_png=True), args.window)
      ms_s2, _ = timed(lambda: net.fusion.feature_extraction(fi, rgb), args.window)
      d4, c4 = disp.view(F, 6, H, W), conf.view(F, 6, H, W)
      ms_six, _ = timed(lambda: six_calls(d4, c4), args.window)
      assert torch.equal(six_calls(d4, c4)[:, 0::2], HG.disp2depth_frames_gpu(disp, conf)[:, 0::2])
    static = frames.clone()
    step = GraphedStep(lambda: net(static), static_inputs=(static,))
    ms_graph, n_graph = timed(step.replay, args.window)
    eager_out = net(frames)
    same = bool(torch.equal(step.replay(), eager_out))
    del step
    torch.cuda.synchronize()
    row = {'frames': F, 'eager_ms': ms_eager, 'eager_ms_per_frame': ms_eager / F, 'eager_calls_timed': n_eager,
           'replay_ms': ms_graph, 'replay_ms_per_frame': ms_graph / F, 'replay_calls_timed': n_graph, 'replay_equals_eager': same,
           'stage1_ms': ms_s1, 'handoff_ms': ms_ho, 'stage2_ms': ms_s2, 'six_call_handoff_ms': ms_six,
           'handoff_speedup': ms_six / ms_ho, 'wall_s': time.time() - t0}
    print(json.dumps(row), flush=True)
    rows.append(row)
    del frames, left, right, rgb, disp, conf, fi, static
    torch.cuda.empty_cache()
  out = {'tool': 'tools/multiview_bench.py', 'size': [H, W], 'maxdisp': MAXDISP, 'window_s': args.window,
         'device': torch.cuda.get_device_name(0), 'torch': torch.__version__, 'rows': rows, 'scoring': scoring_line()}
  os.makedirs(os.path.dirname(args.out), exist_ok=True)
  with open(args.out, 'w') as f:
    json.dump(out, f, indent=1)
  print('wrote', args.out)


if __name__ == '__main__':
  main()
