"""MODE on MI355X: same import surface as the reference's models/__init__.py:1-3 -- the disparity stage (the hot path) and the
fusion stage's ModeFusion / Baseline -- and ModeMultiView, both stages on whole four-camera frames."""
from .mode_disparity import ModeDisparity
from .mode_fusion import ModeFusion, Baseline
from .initModel import initModelPara, loadStackHourglassOnly
from .mode_multiview import ModeMultiView
