"""ModeMultiView: fused 360-degree depth of whole Deep360 frames in one call (forward / evaluate: inference; fusion_loss: training).

The reference runs MODE as two scripts joined through the disk: save_output_disparity_stage.py evaluates one stereo pair at a time
and writes a depth map (.npz) and an 8-bit confidence map (.png) per pair; test_fusion.py reads them back into the fusion network.
Here the chain stays on the GPU:

  stage 1   ONE ModeDisparity(out_conf=True) call over the six pairs of all F frames (batch 6F)
  hand-off  utils.geometry.disp2depth_frames_gpu: depth and confidence of every pair in camera 1's Cassini frame, interleaved as
            ModeFusion takes them (three launches; bit for bit what six disp2depth_gpu calls and a cat give)
  stage 2   the fusion network's feature extraction on the hand-off and the RGB of cameras 1-4

forward() returns (F, 1, H, W) depth in camera 1's Cassini frame; utils.geometry.cassini2Equirec(depth) gives the equirectangular
(F, W, 2W) panorama.  conf_png=True (the default) feeds the fusion network the confidence as the reference's PNG export reads back,
which is what the fusion checkpoints were trained and tested on.

evaluate() goes one step further, to what test_fusion.py:76-100 reports: the ERP panorama and the per-frame metric rows against a
ground truth, scored on the GPU (utils.panorama).

Frames may also arrive as they decode: (F, 12, H, W, 3) uint8 on the device.  Normalisation and the split are then one kernel
(dataloader.gpu_ingest.frames_u8_gpu) and the result is bit for bit that of the float path on the host-normalised frames.  8-bit
frames are what resize=True needs: the reference's --resize path (train_fusion.py / test_fusion.py --resize,
dataloader/deep360_loader.py:146-155) runs the fusion network at half size, on every second pixel of the hand-off and on the RGB
panoramas halved by PIL.Image.resize -- 8-bit fixed-point arithmetic, reproduced on the GPU bit for bit (rgb_half_gpu) -- and
upsamples the result x2 (test_fusion.py:82)."""
import os

import torch
import torch.nn as nn

from dataloader import gpu_ingest
from mode_hip import functional as HF
from mode_hip import require_gpu
from utils import geometry, panorama

from .mode_disparity import ModeDisparity
from .mode_fusion import Baseline, ModeFusion

# panoramas of a frame that the fusion network sees: both images of pair 12 (cameras 1, 2) and both of pair 34 (cameras 3, 4), at
# positions 0, 1, 10, 11 of the frame's 12 files (dataloader/list_file.py _FUSION_RGB)
FUSION_RGB = (0, 1, 10, 11)


def split_frames(frames, rig=None):
  """(F, 12, 3, H, W) panoramas in a frame's sorted file order -> (left (6F, 3, H, W), right (6F, 3, H, W), rgb (F, 12, H, W)).
  Pair p of frame f is left[6f + p] = frames[f, 2p], right[6f + p] = frames[f, 2p + 1] (list_file.py _disparity_subset); rgb is
  frames[f, FUSION_RGB] with the colour channels flattened.  Works on any device.
  rig: a utils.rig.CameraRig of P pairs -> frames (F, 2P, 3, H, W), left, right (P F, 3, H, W), rgb (F, 3 len(rig.rgb), H, W) of the
  panoramas rig.rgb."""
  if rig is not None:
    P = len(rig.pairs)
    if frames.dim() != 5 or frames.shape[1] != 2 * P or frames.shape[2] != 3:
      raise ValueError('ModeMultiView: frames of a rig with %d pairs must be (F, %d, 3, H, W), got %s' % (P, 2 * P, tuple(frames.shape)))
    F, _, C, H, W = frames.shape
    return (frames[:, 0::2].reshape(F * P, C, H, W), frames[:, 1::2].reshape(F * P, C, H, W), torch.cat([frames[:, k] for k in rig.rgb], 1))
  if frames.dim() != 5 or frames.shape[1] != 12 or frames.shape[2] != 3:
    raise ValueError('ModeMultiView: frames must be (F, 12, 3, H, W), got %s' % (tuple(frames.shape),))
  F, _, C, H, W = frames.shape
  left = frames[:, 0::2].reshape(F * 6, C, H, W)
  right = frames[:, 1::2].reshape(F * 6, C, H, W)
  rgb = torch.cat([frames[:, k] for k in FUSION_RGB], 1)  # (no index tensor: an upload cannot be captured into a graph)
  return left, right, rgb


def fusion_size_multiple(fusion):
  """The multiple of which the fusion network's input height and width must be: every nn.MaxPool2d(2) on its deepest path halves
  the map (floor) and the 2x2 transposed convolutions double it back, so the skip connections only line up when the input divides by
  2^(number of poolings) -- 8 for ModeFusion (three poolings on the depth branch), 1 for Baseline (none)."""
  net = fusion.feature_extraction
  pools = sum(isinstance(m, nn.MaxPool2d) for name, m in net.named_modules() if name.startswith('depth_layer'))
  return 2 ** pools


def _state_dict_of(src):
  """A path or a dict in the format of the reference's training scripts ({'state_dict': ...}, keys with or without the
  DataParallel 'module.' prefix) -> a plain state_dict."""
  if isinstance(src, (str, os.PathLike)):
    src = torch.load(src, map_location='cpu')
  sd = src.get('state_dict', src) if isinstance(src, dict) else src
  return {(k[len('module.'):] if k.startswith('module.') else k): v for k, v in sd.items()}


class ModeMultiView(nn.Module):
  """Both MODE stages on whole frames.  Children: `disparity` (ModeDisparity with the confidence output) and `fusion` (ModeFusion,
  or Baseline with fusion='Baseline'), so the state_dict is theirs under the prefixes 'disparity.' and 'fusion.'.
  handoff_grad selects what fusion_loss fine-tunes stage 1 through when disparity.train(): 'depth' (the default) the depth channels of the
  hand-off alone; 'full' the confidence channels as well (needs conf_png=False with ModeFusion) and, with resize=True, the decimation.
  It changes nothing else: forward(), evaluate(), fusion_loss with disparity.eval() and the state_dict do not depend on it.
  rig: a utils.rig.CameraRig instead of dbname (None: the Deep360 frame of 12 panoramas, as above).  A frame is then the rig's 2P
  panoramas, pair-major, (F, 2P, 3, H, W) float or (F, 2P, H, W, 3) uint8; stage 1 runs at batch P F, the hand-off on
  mode_multiview_rig_handoff, and ModeFusion is built for 2P depth / confidence planes and 3 len(rig.rgb) colour planes, so its first
  two layers (and only they) have other shapes than the reference's checkpoints.  Everything else reads as above with 6 -> P."""

  def __init__(self, maxdisp=192, maxdepth=1000., height=1024, width=512, dbname='Deep360', fusion='ModeFusion',
               channels=(32, 64, 128, 256), conf_png=True, resize=False, handoff_grad='depth', rig=None):
    super(ModeMultiView, self).__init__()
    if rig is not None:
      if dbname != 'Deep360':
        raise ValueError('ModeMultiView: rig= and dbname=%r are two descriptions of the cameras; pass one' % (dbname,))
      if fusion == 'Baseline' and len(rig.pairs) != 6:
        raise ValueError("ModeMultiView(fusion='Baseline') needs a rig of 6 pairs, not %d: the reference's Baseline stack has 6 input "
                         'planes' % len(rig.pairs))
      if resize and not rig.deep360_layout:
        raise ValueError('ModeMultiView(resize=True) needs a rig whose frames have the layout of Deep360 (6 pairs, rgb = (0, 1, 10, 11)), '
                         'not %d pairs with rgb = %r: the halving of the 8-bit RGB (mode_rgb_half_pil) reads exactly those panoramas' %
                         (len(rig.pairs), rig.rgb))
    self.rig = rig
    self.pairs = 6 if rig is None else len(rig.pairs)
    if handoff_grad not in ('depth', 'full'):
      raise ValueError("ModeMultiView: handoff_grad must be 'depth' or 'full', not %r" % (handoff_grad,))
    if handoff_grad == 'full' and fusion == 'ModeFusion' and conf_png:
      raise ValueError("ModeMultiView(handoff_grad='full') needs conf_png=False: with conf_png=True the fusion network reads the confidence "
                       'through the rounding to 8 bits of the PNG export, which is piecewise constant and passes no gradient')
    self.handoff_grad = handoff_grad
    if height % 16 or width % 16:
      raise ValueError('ModeMultiView: %d x %d is not a multiple of 16 (the reference pads to 16; this module does not)' % (height, width))
    if fusion not in ('ModeFusion', 'Baseline'):
      raise ValueError('ModeMultiView: fusion must be ModeFusion or Baseline, not %r' % (fusion,))
    geometry._baselines(dbname)  # 3D60 has no baselines in the reference: refused here, not at the first frame
    self.height, self.width, self.dbname, self.conf_png, self.fusion_kind = height, width, dbname, conf_png, fusion
    self.resize = bool(resize)
    self.maxdepth = float(maxdepth)
    self.disparity = ModeDisparity(maxdisp, 'Sphere', height, width, 'Cassini', out_conf=True)
    if fusion == 'ModeFusion':
      self.fusion = ModeFusion(maxdepth, list(channels),
                               {'depth': 12, 'rgb': 12} if rig is None else {'depth': 2 * len(rig.pairs), 'rgb': 3 * len(rig.rgb)})
    else:
      self.fusion = Baseline(maxdepth)
    if self.resize:
      m = 2 * fusion_size_multiple(self.fusion)
      if height % m or width % m:
        raise ValueError('ModeMultiView(resize=True): %d x %d is not a multiple of %d: the fusion network runs at half size, and %s takes '
                         'sizes that its %d poolings halve exactly' % (height, width, m, fusion, (m // 2).bit_length() - 1))

  def load_checkpoints(self, disp=None, fusion=None):
    """Load the checkpoints of the two training scripts (paths or dicts); either may be None."""
    if disp is not None:
      self.disparity.load_state_dict(_state_dict_of(disp))
    if fusion is not None:
      self.fusion.load_state_dict(_state_dict_of(fusion))
    return self

  def _ingest(self, frames):
    """The checks and the split that forward() and fusion_loss() share: frames -> (left, right (6F, 3, H, W), rgb (F, 12, H, W) or None,
    whether the fusion network takes the RGB)."""
    u8 = frames.dtype == torch.uint8
    if self.resize and not u8:
      raise ValueError('ModeMultiView(resize=True) takes uint8 frames (F, 12, H, W, 3), not %s: the reference halves the 8-bit images '
                       '(PIL.Image.resize, fixed-point arithmetic on bytes), and that result cannot be reproduced from normalised '
                       'floats' % (frames.dtype,))
    require_gpu(frames)
    want_rgb = self.fusion_kind == 'ModeFusion'
    if u8:
      left, right, rgb = gpu_ingest.frames_u8_gpu(frames.contiguous(), want_rgb=want_rgb and not self.resize, rig=self.rig)
      H, W = frames.shape[2:4]
    else:
      left, right, rgb = split_frames(frames, self.rig)
      H, W = frames.shape[-2:]
    if H % 16 or W % 16:
      raise ValueError('ModeMultiView: %d x %d is not a multiple of 16' % (H, W))
    if (H, W) != (self.height, self.width):
      raise ValueError('ModeMultiView: built for %d x %d, got %d x %d' % (self.height, self.width, H, W))
    return left, right, rgb, want_rgb

  def forward(self, frames, return_stages=False):
    """frames (F, 12, 3, H, W) float32: ImageNet-normalised panoramas of F frames in sorted file order, or (F, 12, H, W, 3) uint8: the
    same panoramas as they decode -> depth (F, 1, H, W) in camera 1's Cassini frame; with return_stages also {'disp', 'conf':
    (6F, 1, H, W) of stage 1, 'fusion_input': the hand-off}.  resize=True (uint8 frames only): the fusion network runs at half size
    and its output is upsampled x2; the stages then hold the half-size 'fusion_input' and 'rgb' the network saw."""
    if self.training:
      raise RuntimeError('ModeMultiView is inference only: call .eval() first')
    left, right, rgb, want_rgb = self._ingest(frames)
    with torch.no_grad():
      disp, conf = self.disparity(left, right)
      fusion_input = geometry.disp2depth_frames_gpu(disp, conf, self.dbname, conf_png=self.conf_png,
                                                    depth_only=self.fusion_kind == 'Baseline', rig=self.rig)
      if self.resize:  # deep360_loader.py:146-155 on the hand-off and the 8-bit panoramas; test_fusion.py:82 on the result
        fusion_input = HF.decimate2(fusion_input)
        rgb = gpu_ingest.rgb_half_gpu(frames.contiguous()) if want_rgb else None
      if self.fusion_kind == 'ModeFusion':
        depth = self.fusion.feature_extraction(fusion_input, rgb)
      else:
        depth = self.fusion.feature_extraction(fusion_input)
      if self.resize:
        depth = panorama.bicubic_up2(depth)
    if return_stages:
      stages = {'disp': disp, 'conf': conf, 'fusion_input': fusion_input}
      if self.resize:
        stages['rgb'] = rgb
      return depth, stages
    return depth

  def evaluate(self, frames, gt, maxdepth=None):
    """forward(frames), float or uint8, scored as test_fusion.py:86-100 scores a batch: gt (F, H, W) Cassini ground truth on the device ->
    (depth_erp (F, W, H) device panorama, metrics (F, 8) float64 numpy rows [mae, rmse, absrel, sqrel, silog, delta 1, 2, 3] over the
    ERP pixels with gt <= maxdepth; default: the maxdepth the module was built with).  Inference only, like forward()."""
    if self.training:
      raise RuntimeError('ModeMultiView is inference only: call .eval() first')
    require_gpu(frames, gt)
    want = (frames.shape[0], self.height, self.width)
    if tuple(gt.shape) != want:
      raise ValueError('ModeMultiView.evaluate: gt %s is not (F, H, W) = %s' % (tuple(gt.shape), want))
    depth = self.forward(frames)
    rows, depth_erp, _ = panorama.erp_depth_metrics(depth, gt, self.maxdepth if maxdepth is None else maxdepth, return_erp=True)
    return depth_erp, rows

  def fusion_loss(self, frames, gt, lamda=0.5, maxdepth=None):
    """The body of the reference's fusion training iteration between zero_grad() and backward() (train_fusion.py:90-112), on frames:
        output = model(depthes, confs, rgbs);  mask = gt <= maxdepth;  loss = silog_loss(lamda, output[mask], gt[mask])
    frames as forward() takes them, gt (F, H, W) Cassini ground truth on the device -> (loss, depth.detach()).  An extension (the
    reference trains from exported files), after the precedent of ModeDisparity.forward_loss.  The fusion network must be in training
    mode; the state of `disparity` selects what is trained:
      disparity.eval()   the reference's recipe (net.train(); net.disparity.eval()): stage 1 runs without a gradient exactly as in
                         forward(), the hand-off and the fusion network with autograd.  resize=True is taken as
                         Deep360DatasetFusion(resize=True, training=True) takes it: hand-off decimated, 8-bit RGB halved, gt[:, ::2, ::2],
                         no upsampling of the output.
      disparity.train()  joint fine-tuning: the disparity of the third head with its gradient (BatchNorm on the statistics of the batch
                         of 6F pairs), the confidence from the same logits without one, and the gradient of the loss reaches every
                         stage-1 parameter through the hand-off's backward (utils.geometry.disp2depth_frames_gpu).  resize=True is
                         refused under handoff_grad='depth', where the decimation has no backward.
                         handoff_grad='full': disparity and confidence from ONE head pass with a gradient for both
                         (HF.head_conf), the hand-off with conf_grad=True, and resize=True is taken through the differentiable
                         HF.decimate2 (the halving of the 8-bit RGB needs no backward: the frames are data).
    forward() and evaluate() stay inference only."""
    joint, full = self._fusion_training_mode('fusion_loss')
    left, right, rgb, want_rgb = self._ingest(frames)
    require_gpu(gt)
    H, W = left.shape[-2:]
    if tuple(gt.shape) != (left.shape[0] // self.pairs, H, W):
      raise ValueError('ModeMultiView.fusion_loss: gt %s is not (F, H, W) = %s' % (tuple(gt.shape), (left.shape[0] // self.pairs, H, W)))
    output = self._fusion_training_output(frames, left, right, rgb, want_rgb, joint, full)
    if self.resize:  # deep360_loader.py:146-155 with training=True
      gt = gt[:, ::2, ::2]
    loss = HF.silog_loss(output, gt, gt <= (self.maxdepth if maxdepth is None else maxdepth), lamda)
    return loss, output.detach()

  def _fusion_training_mode(self, who):
    """What fusion_loss and fusion_selfsup_loss check before they touch the frames -> (joint, full)."""
    if not self.fusion.training:
      raise RuntimeError('ModeMultiView.%s is the training step of the fusion network: call .train() first '
                         '(.disparity.eval() afterwards keeps stage 1 frozen)' % who)
    joint = self.disparity.training
    full = joint and self.handoff_grad == 'full'
    if joint and self.resize and not full:
      raise ValueError("ModeMultiView(resize=True, handoff_grad='depth').%s cannot fine-tune the disparity stage: on this path "
                       "the decimation of the hand-off has no backward; build the module with handoff_grad='full', or call "
                       '.disparity.eval() to train the fusion network alone' % who)
    return joint, full

  def _fusion_training_output(self, frames, left, right, rgb, want_rgb, joint, full):
    """The chain both training entries share, from the ingested frames to the fusion network's output with its autograd graph
    (stage 1 with or without a gradient as fusion_loss's docstring says, the hand-off, the decimation of resize=True, stage 2)."""
    H, W = left.shape[-2:]
    if full:
      size = (self.disparity.maxdisp, H, W)
      disp, conf = HF.head_conf(self.disparity._logits(left, right)[2], size)
    elif joint:
      size = (self.disparity.maxdisp, H, W)
      cost3 = self.disparity._logits(left, right)[2]
      disp = HF.head(cost3, size)
      conf = HF.head_fwd(cost3.detach(), size, with_confidence=True)[1]
    else:
      with torch.no_grad():
        disp, conf = self.disparity(left, right)
    depth_only = self.fusion_kind == 'Baseline'
    fusion_input = geometry.disp2depth_frames_gpu(disp, conf, self.dbname, conf_png=self.conf_png, depth_only=depth_only,
                                                  conf_grad=full and not depth_only, rig=self.rig)
    if self.resize:  # deep360_loader.py:146-155 with training=True
      fusion_input = HF.decimate2(fusion_input)
      rgb = gpu_ingest.rgb_half_gpu(frames.contiguous()) if want_rgb else None
    if self.fusion_kind == 'ModeFusion':
      return self.fusion.feature_extraction(fusion_input, rgb)
    return self.fusion.feature_extraction(fusion_input)

  def _posed_rig(self, who):
    """The rig whose panorama poses fusion_selfsup_loss and render_views use: self.rig, or Deep360's for dbname='Deep360'."""
    from utils.rig import CameraRig
    if self.rig is not None:
      return self.rig
    if self.dbname != 'Deep360':
      raise ValueError("ModeMultiView(dbname=%r).%s: that setting takes the baselines 0.6 sqrt(2) and 1.2 but keeps the "
                       'unit square\'s translations, so its camera centres are not one rig and the panoramas have no consistent poses; '
                       'build the module with rig=CameraRig.square(0.6 * sqrt(2))' % (self.dbname, who))
    return CameraRig.deep360()

  def fusion_selfsup_loss(self, frames, sources=None, poses=None, visibility=None, **loss_kw):
    """fusion_loss without ground truth: frames exactly as fusion_loss takes them -> (loss, depth.detach()).  The chain is
    fusion_loss's with the SILog term replaced by HF.mv_photometric_loss: the fused depth lives in the common view's Cassini frame, and
    every other panorama of the frame is a picture of the same scene from a pose the rig knows, so each pixel is lifted by its depth,
    projected into the source panoramas and compared there (SSIM + L1, the per-window minimum over the sources, smoothness on log depth).
    The reference image is the frame's own panorama rig.reference_panorama(); sources: panorama indices, default rig.default_sources()
    (one panorama per camera that stands elsewhere), 1 .. 8 of them; their poses are rig.panorama_poses().  rig=None with
    dbname='Deep360' means CameraRig.deep360().  disparity.eval() trains the fusion network alone; disparity.train() fine-tunes stage 1
    through the hand-off, under either handoff_grad.  loss_kw: alpha, lam, beta, mean, std.  The fusion network must be in training mode.
    Refused: resize=True (the loss compares at the frames' own size) and dbname='other' (that setting keeps the unit square's
    translations with other baselines, so its camera centres are not one rig; CameraRig.square(0.6 * sqrt(2)) is).
    poses: (2P, 3, 4) or (2P, 12) float64 on the host, used in place of rig.panorama_poses(); `sources` indexes it as
    before.  With utils.rig_refine.RigRefinement(rig)() the loss's gradient reaches the refinement's twist (the backward then copies
    S x 12 doubles to the host and synchronises); calibrate a source at a time, or only sources that are comparably off: a source
    that loses every window gets no gradient.
    visibility: True, or a dict with tol and / or radius (HF.mv_visibility's; defaults 0.05 and 0): the loss counts a pixel
    for a source only where that source sees it -- the masks are HF.mv_visibility of the detached fused depth of this call with the
    same poses (the detached values of learned ones), constants of every gradient."""
    if self.resize:
      raise ValueError('ModeMultiView(resize=True).fusion_selfsup_loss: the reprojection loss compares the panoramas at their own size, '
                       'and the fusion network runs at half size here; build the module with resize=False')
    rig = self._posed_rig('fusion_selfsup_loss')
    for k in loss_kw:
      if k not in ('alpha', 'lam', 'beta', 'mean', 'std'):
        raise ValueError('fusion_selfsup_loss returns (loss, depth); %r is not a parameter of the loss (alpha, lam, beta, mean, std); call '
                         'HF.mv_photometric_loss for the statistics' % (k,))
    visibility = None if visibility is False else visibility
    if visibility is None or visibility is True:
      vis_kw = {}
    elif isinstance(visibility, dict) and all(k in ('tol', 'radius') for k in visibility):
      vis_kw = dict(visibility)
    else:
      raise ValueError('ModeMultiView.fusion_selfsup_loss: visibility is None, True or a dict with tol and / or radius, got %r' % (visibility,))
    joint, full = self._fusion_training_mode('fusion_selfsup_loss')
    ref_index = rig.reference_panorama()
    sources = rig.default_sources() if sources is None else tuple(int(k) for k in sources)
    if not 1 <= len(sources) <= 8 or any(not 0 <= k < 2 * len(rig.pairs) for k in sources):
      raise ValueError('ModeMultiView.fusion_selfsup_loss: sources %r must be 1 .. 8 panorama indices in [0, %d)' % (sources, 2 * len(rig.pairs)))
    if poses is None:
      poses = rig.panorama_poses()[list(sources)]
    else:
      if not isinstance(poses, torch.Tensor):
        poses = torch.as_tensor(poses, dtype=torch.float64)
      if tuple(poses.shape) not in ((2 * len(rig.pairs), 3, 4), (2 * len(rig.pairs), 12)):
        raise ValueError('ModeMultiView.fusion_selfsup_loss: poses must be (2P, 3, 4) or (2P, 12) with P = %d pairs, one per panorama as '
                         'rig.panorama_poses() gives them, got %s' % (len(rig.pairs), tuple(poses.shape)))
      poses = poses.reshape(2 * len(rig.pairs), 12)[list(sources)]
    left, right, rgb, want_rgb = self._ingest(frames)
    P = self.pairs
    H, W = left.shape[-2:]

    def panorama(k):  # panorama 2p / 2p + 1 of frame f is left / right[P f + p]
      return (left, right)[k % 2].reshape(-1, P, 3, H, W)[:, k // 2]

    ref = panorama(ref_index)
    src = torch.stack([panorama(k) for k in sources], 1)
    output = self._fusion_training_output(frames, left, right, rgb, want_rgb, joint, full)
    if visibility is None:
      loss = HF.mv_photometric_loss(ref, src, output, poses, **loss_kw)
    else:
      loss = HF.mv_photometric_loss(ref, src, output, poses, masks=HF.mv_visibility(output.detach(), poses, **vis_kw), **loss_kw)
    return loss, output.detach()

  def render_views(self, frames, poses, erp=False, **render_kw):
    """What the fused depth map means, shown: frames as forward() takes them, poses (T, 12) or (T, 3, 4) [A | o] of the views
    to render (utils.rig.view_pose(centre, rotation); any T) -> (rendered (F, T, 3, H, W), range (F, T, H, W), hit (F, T, H, W) uint8):
    the frame's own panorama rig.reference_panorama() -- the image the fused depth map is a depth map of, normalised as the frames are
    -- seen from each pose through forward()'s depth, by HF.mv_render.  render_kw: tol, fill, mode.  Runs under no_grad with every
    module in eval mode, whatever mode they are in, and leaves their modes as they were.  erp=True: rendered and range go through
    utils.geometry.cassini2Equirec, (F, T, 3, W, H) and (F, T, W, H); hit stays in the Cassini frame.  Refused: resize=True and
    dbname='other', as fusion_selfsup_loss refuses them."""
    if self.resize:
      raise ValueError('ModeMultiView(resize=True).render_views: the depth map is rendered with the panorama at its own size; build the '
                       'module with resize=False')
    rig = self._posed_rig('render_views')
    for k in render_kw:
      if k not in ('tol', 'fill', 'mode'):
        raise ValueError('render_views returns (rendered, range, hit); %r is not a parameter of the render (tol, fill, mode); call '
                         'HF.mv_render for the index' % (k,))
    ref_index = rig.reference_panorama()
    modes = [(m, m.training) for m in self.modules()]
    self.eval()
    try:
      with torch.no_grad():
        depth = self.forward(frames)
        left, right, _, _ = self._ingest(frames)
        H, W = left.shape[-2:]
        ref = (left, right)[ref_index % 2].reshape(-1, self.pairs, 3, H, W)[:, ref_index // 2]
        rendered, rng, hit = HF.mv_render(ref, depth, poses, return_range=True, return_hit=True, **render_kw)
        if erp:
          F, T = hit.shape[:2]
          rendered = geometry.cassini2Equirec(rendered.reshape(F * T, 3, H, W)).reshape(F, T, 3, W, H)
          rng = geometry.cassini2Equirec(rng.reshape(F * T, 1, H, W)).reshape(F, T, W, H)
    finally:
      for m, was in modes:
        m.training = was
    return rendered, rng, hit

  def photometric_loss(self, frames, **loss_kw):
    """Adapt stage 1 to a rig's own images, which come without depth or disparity ground truth: frames exactly as
    fusion_loss takes them, float or uint8, with or without rig= -> (loss, disp.detach()), the loss of
    ModeDisparity.forward_photometric_loss over the P F stereo pairs of the frames and disp (P F, 1, H, W) its third output.  Needs
    disparity.train().  The fusion network is not run and its parameters get no gradient; resize=True changes nothing here (stage 1
    always runs at full size).  loss_kw: weights, alpha, lam, beta, mean, std."""
    if not self.disparity.training:
      raise RuntimeError('ModeMultiView.photometric_loss trains the disparity stage: call .disparity.train() first')
    left, right, _, _ = self._ingest(frames)
    loss, preds = self.disparity.forward_photometric_loss(left, right, **loss_kw)
    return loss, preds[2]

  def selfsup_loss(self, frames, **kw):
    """photometric_loss with the remedy for occlusion: frames exactly as photometric_loss takes them ->
    (loss, disp.detach()), the loss of ModeDisparity.forward_selfsup_loss (both views' photometric terms, their left-right consistency,
    occlusion masks) over the P F stereo pairs and disp (P F, 1, H, W) the left view's third output.  Needs disparity.train(); the
    fusion network is not run and its parameters get no gradient.  kw: weights, lr_weight, tau, occlusion, alpha, lam, beta, mean, std."""
    if not self.disparity.training:
      raise RuntimeError('ModeMultiView.selfsup_loss trains the disparity stage: call .disparity.train() first')
    left, right, _, _ = self._ingest(frames)
    loss, preds, _ = self.disparity.forward_selfsup_loss(left, right, **kw)
    return loss, preds[2]
