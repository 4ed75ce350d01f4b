"""implicit_depth_amd — MI355X-native LIDF per-point implicit-depth query path.

Host-side mirror of the reference interface for this path (names follow the reference):
  decoders.get_embedder / IMNet / IEF        <- models/implicit_net.py
  pointnet.PointNet2Stage                    <- models/pointnet.py
  extensions.ray_aabb.forward / pcl_aabb     <- extensions/{ray_aabb,pcl_aabb}
  query.get_miss_ray / compute_ray_aabb / lidf_query / lidf_refine / get_occ_vox_bound /
        depth_metrics / lidf_query_train     <- models/pipeline.py:162-466, 577-627, 922-1041
  pipeline.lidf_forward / refine_forward     <- LIDF.forward / RefineNet.forward, eval flavour
  pipeline.lidf_forward_train                <- LIDF.forward, exp_type 'train' (one stage-1 training step)
  pipeline.refine_forward_train / train_refine_step  <- RefineNet.forward, exp_type 'train' / the two forward
                                                calls of trainers/train_refine.py:374-393 (one stage-2 training step)
  losses.compute_gt / lidf_loss              <- LIDF.compute_gt / compute_loss ('train', 'valid', 'test'),
                                                models/pipeline.py:298-336, 468-650
  losses.refine_loss                         <- RefineNet.compute_loss ('train', 'valid', 'test'), models/pipeline.py:760-919
  pipeline.eval_loss / FrameRunner.loss_dict <- loss_dict of LIDF.forward / RefineNet.forward for 'valid' / 'test'
                                                (what trainers' validate() / test() read); per_frame=True: the
                                                loss_dict of test() at bs == 1 for every frame of a batch
  losses.frame_slice                         the bs == 1 data_dict of one frame of a batch
  query.depth_metrics_frames                 <- the nine statistics of :577-627 for every frame of a batch
  losses.topk_mean                           <- torch.topk + mean of hard-negative mining, :475-490, 767-770
  torch_ext.ext()                            <- the pybind11 operator module (extensions/*/jit.py)
All compute goes through csrc/liblidf_hip.so (C ABI in include/lidf_hip.h).
"""
from . import _lib  # noqa: F401
from .decoders import (IEF, IMNet, Embedder, decoders_forward, decoders_forward_train,  # noqa: F401
                       get_embedder)
from .pointnet import PointNet2Stage  # noqa: F401
from .losses import (LidfLossOptions, compute_gt, frame_slice, lidf_loss, lidf_loss_composite,  # noqa: F401
                     refine_loss, refine_loss_composite, topk_mean)
from .pipeline import (LidfOptions, eval_loss, lidf_forward_train, refine_forward_train,  # noqa: F401
                       train_refine_step)

__all__ = ["IEF", "IMNet", "Embedder", "PointNet2Stage", "decoders_forward", "decoders_forward_train",
           "get_embedder", "LidfLossOptions", "LidfOptions", "compute_gt", "lidf_loss", "lidf_loss_composite",
           "lidf_forward_train", "refine_loss", "refine_loss_composite", "topk_mean", "refine_forward_train", "train_refine_step",
           "eval_loss", "frame_slice"]
