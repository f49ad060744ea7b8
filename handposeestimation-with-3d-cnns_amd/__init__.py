"""MI355X-native projective-TSDF voxelizer (drop-in for the reference's
pre/tsdf_numba.py / pre/tsdf_for.py / pre/process.py voxelization path).

The compute path is the hand-written HIP library ``libtsdf_hip.so`` (csrc/tsdf_hip.hip)
behind the C ABI of include/tsdf.h.  Nothing here falls back to a CPU implementation.

Batched API (torch tensors on the GPU):  voxelize, voxelize_grid, voxelize_aug (fused 3-D augmentation), aabb
Augmentation drawn on the GPU:           aug_xforms (libtsdf_augment.so, include/tsdf_augment.h), ResidentLoader(augment="device")
... from counters in device memory:      aug_xforms_at, aug_state, AugmentedStep (libtsdf_augstep.so, include/tsdf_augstep.h),
                                         MSRA_Dataset(aug="device"), ResidentLoader(augment="device", graph=True)
Reference-signature shims:               tsdf_numba.cal_tsdf_cuda, tsdf_for.tsdf_f / tsdf_cal,
                                         process.DataProcess
Host side:                               packing (MSRA .bin reader / batch packer), shard, synth,
                                         dataset (on-the-fly MSRADepthDataset / VoxelLoader / ResidentLoader, label normalisation)
Full mode and evaluation:                pca (JointPCA, fit_joint_pca), project_joints, pose_error, joints_within,
                                         frames_within
Point clouds:                            point_clouds (back-projected, resampled on the device), export.preprocess_tree
The reference's process(), batched:      cloud_grids (grid placed on a cloud's extremes), process_batch (point_clouds ->
                                         cloud_grids -> voxelize_grid)
... and its augmented half:              voxelize_aug_grid (the augmented voxelizer on a caller-supplied grid), transform_joints
                                         (libtsdf_auggrid.so, include/tsdf_auggrid.h), process_batch_aug
Packs with 16-bit depth:                 packing.depth16_shift, PackedFrames.to_depth16 / to_float32 (TSDFPK02, lossless or
                                         refused), widen_depth16 (libtsdf_depth16.so, include/tsdf_depth16.h); the loaders
                                         upload uint16 and widen on the GPU
Volumes in the cloud's principal axes:   obb_xforms (per-frame OBB maps from the depth alone: libtsdf_obb.so,
                                         include/tsdf_obb.h), voxelize_obb, invert_xforms, ResidentLoader(frame="obb")
Volumes in float16 / bfloat16:           voxelize_grid_lowp (the plain voxel pass narrowed in registers: libtsdf_lowp.so,
                                         include/tsdf_lowp.h), voxelize_lowp, narrow_volumes, process_batch(dtype=...),
                                         ResidentLoader(volume_dtype=...)
... under a per-frame map:               map_grids (the map's grid placement on its own), voxelize_map_grid_lowp (the
                                         augmented voxel pass narrowed in registers: libtsdf_maplowp.so,
                                         include/tsdf_maplowp.h), voxelize_aug_lowp, voxelize_obb(dtype=...),
                                         process_batch_aug(dtype=...), AugmentedStep(dtype=...)
Augmentation in a base (OBB) frame:      compose_xforms (two per-frame maps as one), map_step_head (draw, compose, grid
                                         placement and labels in one launch: libtsdf_mapstep.so, include/tsdf_mapstep.h),
                                         AugmentedStep(base=..., fused_head=...)
Raw frames without a bounding box:       locate_hands (the nearest object's centre of mass, a fixed cube about it, the crops
                                         packed as depth / offsets / headers: libtsdf_locate.so, include/tsdf_locate.h),
                                         voxelize_frames (placement="aabb" | "cube")
The accurate directional TSDF:           voxelize_grid_accurate (per voxel the nearest surface point among ALL valid pixels:
                                         libtsdf_accurate.so, include/tsdf_accurate.h), voxelize_accurate,
                                         voxelize_frames(tsdf="accurate"), export.preprocess_tree(tsdf="accurate")
... under a per-frame map:               voxelize_map_grid_accurate (the same search on the augmented pass's arithmetic:
                                         libtsdf_mapaccurate.so, include/tsdf_mapaccurate.h), voxelize_aug_accurate,
                                         voxelize_obb(tsdf="accurate"), AugmentedStep(tsdf="accurate")
Voxel heatmap labels:                    joint_heatmaps (one Gaussian volume per joint from gt_nor, aligned with the TSDF
                                         volume: libtsdf_heatmap.so, include/tsdf_heatmap.h), heatmap_joints (per joint the
                                         peak of a volume back as normalised coordinates), AugmentedStep(heatmap=...)
Voxel heatmap training:                  heatmap_mse_loss (the squared error against joint_heatmaps' targets without the
                                         targets in memory, with its gradient: libtsdf_heatloss.so,
                                         include/tsdf_heatloss.h), soft_argmax_joints (the expectation under a softmax of
                                         the whole volume as normalised coordinates, with its gradient); both are
                                         torch.autograd.Functions, differentiable in the prediction
Occupancy volumes:                       occupancy_volumes (the one-channel input of V2V-PoseNet and its family on the cube
                                         of any placement, every pixel scattered into a bit mask in LDS:
                                         libtsdf_occupancy.so, include/tsdf_occupancy.h), voxelize_occupancy (placed on the
                                         cloud's own cube), AugmentedStep(occupancy=...)
Farthest-point sampled clouds:           farthest_points (the input of a point network — HandPointNet and its family — from
                                         a packed crop, optionally under per-frame maps such as obb_xforms': one workgroup
                                         per frame runs the whole chain of arg-max reductions on chip: libtsdf_fps.so,
                                         include/tsdf_fps.h), farthest_of (of clouds that exist already), FpsBatch, fps_plan,
                                         FPS_RESIDENT_POINTS (the candidates a frame may have without a workspace),
                                         AugmentedStep(fps=...)
kNN grouping and surface normals:        knn_groups (for every centre of a set-abstraction level its k nearest neighbours in
                                         the sampled cloud, the centres a prefix of the cloud: a top-K selection per query
                                         over a cloud resident in LDS, ties to the lowest row: libtsdf_group.so,
                                         include/tsdf_group.h), point_normals (PCA normals over the same neighbours, turned
                                         towards the viewpoint, with the surface variation), KnnBatch, NormalBatch,
                                         group_plan, AugmentedStep(fps=..., groups=..., normals=...)
Point-wise offset fields:                point_fields (the labels of a point-to-point regression network: per sampled point
                                         and joint a heat and a unit vector towards the joint, on the joint's k nearest
                                         points inside a ball — a radix select per joint over a cloud resident in LDS:
                                         libtsdf_pointfield.so, include/tsdf_pointfield.h), field_joints (each joint back
                                         from a predicted field by a weighted vote of its points of greatest heat),
                                         PointFieldBatch, FieldJoints, pointfield_plan, AugmentedStep(fps=..., fields=...)
Depth-image patches (the 2-D CNN input): frame_patches (per located cube a fixed-size [n, 1, S, S] patch resampled from the
                                         cube's image rectangle in raw frames, depth normalised by the cube to [-1, 1],
                                         background +1, nearest or bilinear without blending hand and background, under an
                                         optional in-plane map per frame: libtsdf_patch.so, include/tsdf_patch.h),
                                         crop_patches (the same on a pack), patch_affines (rotation / scale / shift maps),
                                         joints_to_uvd and uvd_to_joints (the joints in the patch's coordinates and back),
                                         patch_frames (locate_hands chained into the three), PatchBatch, UvdBatch, patch_plan
"""
from . import _lib  # noqa: F401
from ._lib import TsdfCam, TsdfError, default_cam  # noqa: F401
from .voxelize import (AabbBatch, AugmentedStep, CloudGridBatch, MapGridBatch, ObbBatch, PointCloudBatch, PoseError, ProcessAugBatch, ProcessBatch, TsdfBatch,  # noqa: F401
                       aabb,
                       aug_state, aug_xforms, aug_xforms_at, cloud_grids, denormalize_joints, empty_batch,
                       frames_within, joints_within, normalize_joints, point_clouds, pose_error, process_batch, process_batch_aug,
                       project_joints, release_stream, transform_joints, voxel_pixels, voxelize_aug_grid,
                       voxelize, voxelize_aug, voxelize_grid, voxelize_indexed, voxelize_labels, widen_depth16,
                       invert_xforms, obb_xforms, voxelize_obb, narrow_volumes, voxelize_grid_lowp, voxelize_lowp,
                       map_grids, voxelize_aug_lowp, voxelize_map_grid_lowp, MapStepBatch, compose_xforms, map_step_head,
                       HandCrops, locate_hands, voxelize_frames, voxelize_accurate, voxelize_grid_accurate,
                       voxelize_aug_accurate, voxelize_map_grid_accurate, HeatmapJoints, heatmap_joints, joint_heatmaps,
                       heatmap_mse_loss, soft_argmax_joints, occupancy_volumes, voxelize_occupancy, FpsBatch,
                       farthest_points, farthest_of, fps_plan, KnnBatch, NormalBatch, knn_groups,
                       point_normals, group_plan, PointFieldBatch, FieldJoints, point_fields, field_joints,
                       pointfield_plan, PatchBatch, UvdBatch, frame_patches, crop_patches, joints_to_uvd,
                       uvd_to_joints, patch_affines, patch_frames, patch_plan)
from .pca import JointPCA, fit_joint_pca  # noqa: F401
from . import augment, dataset, export, packing, pca, shard, synth  # noqa: F401
from .dataset import MSRA_Dataset, MSRADepthDataset, ResidentLoader, VoxelBatch, VoxelLoader  # noqa: F401
from .tsdf_numba import cal_tsdf_cuda  # noqa: F401
from .tsdf_for import tsdf_cal, tsdf_f  # noqa: F401
from .process import DataProcess  # noqa: F401

__all__ = ["voxelize", "voxelize_labels", "voxelize_indexed", "ResidentLoader", "voxel_pixels", "release_stream", "voxelize_grid", "voxelize_aug", "augment", "aabb", "TsdfBatch", "AabbBatch", "TsdfCam", "TsdfError",
           "default_cam", "cal_tsdf_cuda", "tsdf_f", "tsdf_cal", "DataProcess", "packing", "shard",
           "synth", "dataset", "MSRADepthDataset", "MSRA_Dataset", "VoxelLoader", "VoxelBatch", "normalize_joints", "denormalize_joints",
           "pca", "JointPCA", "fit_joint_pca", "project_joints", "pose_error", "PoseError", "joints_within", "frames_within",
           "point_clouds", "PointCloudBatch", "cloud_grids", "CloudGridBatch", "process_batch", "ProcessBatch", "aug_xforms",
           "aug_xforms_at", "aug_state", "AugmentedStep", "voxelize_aug_grid", "transform_joints", "process_batch_aug",
           "ProcessAugBatch", "widen_depth16", "obb_xforms", "voxelize_obb", "invert_xforms", "ObbBatch",
           "voxelize_grid_lowp", "voxelize_lowp", "narrow_volumes", "map_grids", "MapGridBatch", "voxelize_map_grid_lowp",
           "voxelize_aug_lowp", "compose_xforms", "map_step_head", "MapStepBatch", "locate_hands", "voxelize_frames",
           "HandCrops", "voxelize_grid_accurate", "voxelize_accurate", "voxelize_map_grid_accurate", "voxelize_aug_accurate",
           "joint_heatmaps", "heatmap_joints", "HeatmapJoints", "heatmap_mse_loss", "soft_argmax_joints",
           "occupancy_volumes", "voxelize_occupancy", "farthest_points", "farthest_of", "FpsBatch", "fps_plan",
           "FPS_RESIDENT_POINTS", "knn_groups", "point_normals", "KnnBatch", "NormalBatch", "group_plan",
           "point_fields", "field_joints", "PointFieldBatch", "FieldJoints", "pointfield_plan",
           "frame_patches", "crop_patches", "joints_to_uvd", "uvd_to_joints", "patch_affines", "patch_frames", "PatchBatch",
           "UvdBatch", "patch_plan"]


def __getattr__(name):
    if name == "FPS_RESIDENT_POINTS":   # from tsdf_fps_plan, once somebody asks (the library is loaded then, not at import)
        return fps_plan()[0]
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
