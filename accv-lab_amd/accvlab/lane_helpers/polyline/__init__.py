from .ops import interpolate, interpolate_var_size_batch, lengths, lengths_var_size_batch
from .set_prediction import batched_polyline_hungarian_match, batched_polyline_matching_cost, matched_polyline_loss

__all__ = ["interpolate", "interpolate_var_size_batch", "lengths", "lengths_var_size_batch",
           "batched_polyline_matching_cost", "batched_polyline_hungarian_match", "matched_polyline_loss"]
