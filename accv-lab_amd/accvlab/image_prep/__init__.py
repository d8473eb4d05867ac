"""accvlab.image_prep — (extension) the image side of the reference's camera pipeline (packages/dali_pipeline_framework:
AffineTransformer, PhotoMetricDistorter, ImageToTileSizePadder, ImageMeanStdDevNormalizer / ImageRange01Normalizer) as one
HIP launch on the MI355X: ``prepare_images`` and the host-side helpers that build its parameters, among them
``sample_image_transforms`` with the step descriptors of the reference's AffineTransformer (``transforms.py``): the matrices
it returns warp the images here and their annotations in ``accvlab.draw_heatmap.camera_augment_boxes``.  ``nv12.py`` is the
entry of the leg for decoder surfaces: ``nv12_to_rgb`` (the reference's ``convert_nv12_to_rgb``) and ``prepare_images_nv12``,
which reads the NV12 planes directly."""
from .nv12 import nv12_planes, nv12_to_rgb, prepare_images_nv12
from .prepare import (CHANNEL_PERMUTATIONS, IDENTITY_PHOTOMETRIC, MAX_EXTENT, TILE_H, TILE_W, output_size_transform,
                      padded_hw, prepare_images, sample_photometric_params, sample_positions)

from .transforms import (NonUniformScaling, Rotation, Selection, Shearing, ShiftInsideOriginalImage,
                         ShiftToAlignWithOriginalImageBorder, Translation, UniformScaling, sample_image_transforms)

__all__ = ["sample_image_transforms", "Translation", "ShiftInsideOriginalImage", "ShiftToAlignWithOriginalImageBorder",
           "Rotation", "UniformScaling", "NonUniformScaling", "Shearing", "Selection",
           "prepare_images", "prepare_images_nv12", "nv12_to_rgb", "nv12_planes", "sample_photometric_params", "output_size_transform", "padded_hw", "sample_positions",
           "CHANNEL_PERMUTATIONS", "IDENTITY_PHOTOMETRIC", "MAX_EXTENT", "TILE_W", "TILE_H"]
