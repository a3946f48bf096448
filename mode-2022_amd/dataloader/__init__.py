"""Deep360 and 3D60 data access (reference: dataloader/{list_file,preprocess,deep360_loader,dataset3D60Loader}.py).
Host-side IO around the hot path; needs PIL and numpy only (the reference needs cv2 and torchvision).
gpu_ingest is the same work on frames that are already on the device (8-bit ingest, the half-resolution RGB of --resize,
the ERP-to-Cassini ingest of 3D60 pairs with their disparity ground truth, and Deep360 pairs stored at another size than the
working one: resize, crop and disparity ground truth)."""
from . import gpu_ingest, list_file, preprocess
from .list_file import list_deep360_disparity_train, list_deep360_disparity_test, list_deep360_fusion_train, list_deep360_fusion_test
from .list_file import list_deep360_frames
from .deep360_loader import Deep360DatasetDisparity, Deep360DatasetFusion
from .dataset3D60Loader import Dataset3D60Disparity
