"""accvlab.point_cloud — (extension) the lidar side of a detector's preparation step on the MI355X: ``voxelize_points``, the
hard voxelization of a ragged batch of point clouds (mmcv's ``Voxelization`` / spconv's ``points_to_voxel``, called once per
frame in mmdet3d's ``Base3DDetector.voxelize``) with the result of the sequential loop, bit for bit, on the device and on the
host; ``concatenate_voxels`` gives mmdet3d's concatenated form.  ``pillar_features`` (mmdet3d's ``PillarFeatureNet`` up to its
first linear layer) and ``voxel_mean`` (``HardSimpleVFE``) read those voxels in one launch each, and ``scatter_to_bev``
(``PointPillarsScatter``, differentiable) writes the per-pillar features into the dense map of the 2D backbone, once."""
from .bev_scatter import MAX_CHANNELS, scatter_to_bev
from .pillar_features import pillar_features, voxel_mean
from .voxelize import MAX_D, MAX_POINTS, MAX_VOXELS, MIN_D, Voxels, concatenate_voxels, voxelize_points

__all__ = ["voxelize_points", "Voxels", "concatenate_voxels", "pillar_features", "voxel_mean", "scatter_to_bev", "MIN_D", "MAX_D",
           "MAX_POINTS", "MAX_VOXELS", "MAX_CHANNELS"]
