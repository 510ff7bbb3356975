"""Host-side mirror of the reference harness (eval.py loop, GT preparation, depth / normal / point-cloud / camera metrics, CSV sink).
Plain numpy / Python; the model call inside the loop is the only GPU work."""
from .io_utils import prepare_gt_label
from .metrics import (MetricsManager, depth_evaluation, depth_evaluation_in_global_coord, l1_fit, l1_objective, normal_evaluation,
                      pcd_evaluation, pcd_threshold_scores, voxel_iou, world_points_from_depth)
from .camera import camera_pose_evaluation, save_camera_trajectories, tum_poses, write_tum_trajectory
from .pointmap import pointmap_focal, pointmap_poses, poses_from_pointmap
from .temporal import aligned_depth, relative_poses, temporal_alignment_error, warp_depth
from .eval import (evaluate, parse_temporal_eval_config, parse_camera_eval_config, parse_dataset_config, parse_depth_coord, parse_metric_config, parse_pcd_eval_config,
                   import_class_from_module)
from .dataset import SyntheticGeometryDataset, split_clips
from .scannetpp import ScannetPPDataset, ScannetPPSequence
from .rgbd import (RGBDClipDataset, RGBDSequence, ScannetV2Dataset, bonnDataset, neuralRGBDDataset, read_tum_trajectory, replicaDataset,
                   sevenScenesDataset, RegisterOpts, register_depth)
from .distributed import evaluate_sharded
from .ply import read_ply_mesh, write_ply_mesh
from .render import render_mesh, rescaled_size_and_intrinsics
from .vis import SPECTRAL_R_LUT, colorbar_strip, colorize, panels_u8, read_ply, save_depth_normal_maps, write_ply

__all__ = ["prepare_gt_label", "MetricsManager", "depth_evaluation", "depth_evaluation_in_global_coord",
           "l1_fit", "l1_objective", "normal_evaluation", "pcd_evaluation", "pcd_threshold_scores", "voxel_iou", "world_points_from_depth", "evaluate", "parse_dataset_config", "parse_depth_coord",
           "parse_metric_config", "parse_pcd_eval_config", "parse_camera_eval_config", "parse_temporal_eval_config",
           "aligned_depth", "relative_poses", "temporal_alignment_error", "warp_depth", "import_class_from_module", "SyntheticGeometryDataset",
           "split_clips", "evaluate_sharded", "ScannetPPDataset", "ScannetPPSequence",
           "RGBDClipDataset", "RGBDSequence", "sevenScenesDataset", "bonnDataset", "neuralRGBDDataset", "replicaDataset", "ScannetV2Dataset",
           "read_tum_trajectory", "RegisterOpts", "register_depth",
           "camera_pose_evaluation", "tum_poses", "write_tum_trajectory", "save_camera_trajectories",
           "pointmap_focal", "pointmap_poses", "poses_from_pointmap",
           "SPECTRAL_R_LUT", "colorbar_strip", "colorize", "panels_u8", "save_depth_normal_maps", "write_ply", "read_ply",
           "read_ply_mesh", "write_ply_mesh", "render_mesh", "rescaled_size_and_intrinsics"]
