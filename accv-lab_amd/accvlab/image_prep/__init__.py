"""accvlab.image_prep — (extension) the image side of the reference's camera pipeline (packages/dali_pipeline_framework:
AffineTransformer, PhotoMetricDistorter, ImageToTileSizePadder, ImageMeanStdDevNormalizer / ImageRange01Normalizer) as one
HIP launch on the MI355X: ``prepare_images`` and the host-side helpers that build its parameters."""
from .prepare import (CHANNEL_PERMUTATIONS, IDENTITY_PHOTOMETRIC, MAX_EXTENT, TILE_H, TILE_W, output_size_transform,
                      padded_hw, prepare_images, sample_photometric_params, sample_positions)

__all__ = ["prepare_images", "sample_photometric_params", "output_size_transform", "padded_hw", "sample_positions",
           "CHANNEL_PERMUTATIONS", "IDENTITY_PHOTOMETRIC", "MAX_EXTENT", "TILE_W", "TILE_H"]
