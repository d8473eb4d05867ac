/*
 * accv_hip.h — C-ABI of libaccv_hip.so: the MI355X (gfx950) drop-in for the native layer of ACCV-Lab's
 * per-step data/target-preparation hot path.  Plain pointers and sizes only; no torch/ATen types.
 *
 * Conventions
 *   - every entry point returns 0 on success or a negative ACCV_E* code; accv_last_error() returns a
 *     thread-local message for the last failure on the calling thread;
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream); all work is enqueued
 *     asynchronously on it, nothing synchronises, nothing allocates device memory — the caller owns every
 *     buffer including the workspace (hipGraph-capturable, re-entrant);
 *   - device pointers unless a parameter is documented as host memory.
 *
 * Each function cites the reference interface it replaces (paths relative to the ACCV-Lab checkout).
 */
#ifndef ACCV_HIP_H
#define ACCV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACCV_OK 0
#define ACCV_EINVAL (-1)   /* bad argument (shape, null pointer, unsupported dtype code) */
#define ACCV_ELAUNCH (-2)  /* HIP runtime reported an error at launch / enqueue */
#define ACCV_EWORKSPACE (-3) /* workspace too small */
#define ACCV_ERUNTIME (-4) /* other runtime failure (host allocation, thread pool, ...) */

/* flags for the draw_heatmap entry points */
#define ACCV_HM_CLEAR 1u       /* fused clear: result = max(0, splats); every pixel is written exactly once */
#define ACCV_HM_COUNTS_I64 2u  /* `counts` points to int64 (RaggedBatch.sample_sizes) instead of int32 */
#define ACCV_HM_SMALL_RADII 4u /* hint: radii of a few pixels (lane samples, key points; boxes up to ~15x15): take the
                                 kernel that walks each object's box instead of updating whole tiles.  Results do
                                 not depend on the hint; objects of any size stay correct, only slower. */
#define ACCV_HM_WRITE_THROUGH 8u /* hint: write the map with write-through non-temporal stores (sc1 nt) instead of plain
                                    ones.  Pays 1-7 % for launches that rewrite far more than L2 + Infinity Cache hold AND
                                    are compute heavy (dense batches, in-place over most of the frame); costs up to 27 %
                                    for sparse in-place launches, which is why it is not the default.  Same results. */
#define ACCV_HM_GROUP_BOXES_GIVEN 16u /* accv_draw_points_multiscale_f32 only: `workspace` already holds the group boxes
                                         (written by accv_polyline_sample_boxes); skip the box launch */

#define ACCV_HM_PLAIN_STORES 128u /* hint: plain stores for every plane.  Default: fused-clear launches store plain; in-place
                                    launches choose per plane — write-through non-temporal where the plane's objects
                                    cover >= 3/4 of its area (sum of (2r+1)^2), plain elsewhere.  Same results. */
#define ACCV_HM_TILE_ROWS_16 32u /* hint: 128 x 32 pixel wave tiles (half the waves, twice the registers per wave) */
#define ACCV_HM_TILE_ROWS_8 64u  /* hint: 128 x 16 pixel wave tiles (the default).  Same results either way. */
#define ACCV_HM_CALLER_SCALE_ORDER 256u /* multi-scale calls only: keep the caller's order of scales in the launch.  Default:
                                         * coarse scales (fewest tiles, longest per-tile work) are dispatched first.  Same
                                         * results either way. */

const char* accv_last_error(void);
int accv_version(void);
/* Which kernel instantiation and launch geometry the LAST draw_heatmap entry point called on this thread selected
 * (thread-local, e.g. "splat_kernel<PX=4,R=16,CLEAR=1,SM=0> grid(15,34,64) block(64)"); "" before the first call.
 * For benchmarks and profiles: the name a rocprofv3 kernel trace shows for that launch starts with the same text. */
const char* accv_draw_heatmap_last_dispatch(void);

/* ------------------------------------------------------------------------------------------------ H1
 * Gaussian heat-map rasteriser.
 */

/* Profiling aid (no reference counterpart): the splat kernel of the NEXT accv_draw_heatmap_flat_f32 /
 * accv_draw_heatmap_batched_f32 call made by the calling thread records `start_event` when it begins to execute and
 * `stop_event` when it has finished (hipExtLaunchKernel), i.e. the kernel's own duration, without the dispatch gap that
 * separates back-to-back launches on a stream.  Both are hipEvent_t with timing enabled (either may be NULL).  One-shot:
 * that call consumes the pair whether or not it launches (a call that returns early leaves the events unrecorded), and a
 * multi-scale draw call in between drops it; (NULL, NULL) cancels.  bench.py derives roofline.kernel_ms from it; kernel and launch parameters are unchanged. */
int accv_draw_heatmap_time_next_launch(void* start_event, void* stop_event);

/* Replaces draw_heatmap_launcher / draw_heatmap_cuda  (packages/draw_heatmap/accvlab/draw_heatmap/csrc/
 * draw_heatmap_cuda.cu:29-41,62-89; kernel include/draw_heatmap_cuda_kernel.cuh:51-74).
 * heatmaps f32[P,H,W] (in/out), centers i32[N,2] (x,y), radii i32[N], heatmap_idxes i32[N].
 * Objects whose plane index is outside [0,P) are ignored (the reference writes out of bounds).
 * workspace: accv_draw_heatmap_flat_workspace_bytes(P,N) bytes of device memory, 16-byte aligned. */
size_t accv_draw_heatmap_flat_workspace_bytes(int num_planes, int num_objects);
int accv_draw_heatmap_flat_f32(float* heatmaps, int num_planes, int height, int width, const int32_t* centers,
                               const int32_t* radii, const int32_t* heatmap_idxes, int num_objects,
                               float diameter_to_sigma_factor, float k_scale, unsigned flags, void* workspace,
                               size_t workspace_bytes, void* stream);

/* Replaces draw_heatmap_batched_launcher / draw_heatmap_batched_classwise_launcher / draw_heatmap_batched_cuda
 * (draw_heatmap_cuda.cu:43-60,91-124,126-165; kernel cuh:76-108).
 * heatmap f32[B,H,W] (num_classes == 0, labels == NULL) or f32[B,C,H,W] (class-wise);
 * centers i32[B,Nmax,2], radii i32[B,Nmax], labels i32[B,Nmax] or NULL, counts i32[B] (or i64[B] with
 * ACCV_HM_COUNTS_I64 — removes the per-call cast of draw_heatmap_batched.py:63).
 * Labels outside [0,C) are ignored (the reference device-asserts, cuh:102). Needs no workspace. */
int accv_draw_heatmap_batched_f32(float* heatmap, int batch, int num_classes, int height, int width,
                                  const int32_t* centers, const int32_t* radii, const void* counts,
                                  const int32_t* labels, int max_num_targets, float diameter_to_sigma_factor,
                                  float k_scale, unsigned flags, void* stream);

/* Multi-scale target maps in ONE launch (BASELINE config 3; SURVEY §8 f2 fused into H1): for every scale s,
 *   (c, r) = targets_from_boxes(centers_xy, boxes_xyxy, strides[s])   — packages/draw_heatmap/tests/_test_helpers.py:20-28
 *   draw_heatmap_batched(heatmaps[s] f32[batch, heights[s], widths[s]], c, r, counts, factor, k)
 * with the float -> integer conversion done inside the kernel's culling step (no intermediate tensors).  Results are
 * identical to the per-scale calls.  heatmaps / heights / widths / strides are HOST arrays of `num_scales` (<= 4)
 * entries; centers f32[batch, Nmax, 2], boxes f32[batch, Nmax, 4] (source pixels), counts as in the batched call.
 * Every map needs width % 4 == 0, a 16-byte aligned base and planes below 2 GiB (else use the per-scale calls). */
int accv_draw_heatmap_multiscale_f32(float* const* heatmaps, const int* heights, const int* widths, const float* strides,
                                     int num_scales, int batch, const float* centers_xy, const float* boxes_xyxy,
                                     const void* counts, int max_num_targets, float diameter_to_sigma_factor,
                                     float k_scale, unsigned flags, void* stream);

/* accv_draw_heatmap_multiscale_f32 with the polyline sampler riding in the same launch (BASELINE config 3 prepares box maps and
 * lane maps every step; the sampler's few hundred workgroups cost nothing next to the box maps' tiles, a launch of their own
 * costs 5.9 us).  The first 13 arguments are those of accv_draw_heatmap_multiscale_f32 and mean the same; in addition
 * polylines_xy f32[num_polylines, points, 2] (1..64 points; point_counts[num_polylines] valid leading points, int32 or int64
 * with ACCV_HM_POINT_COUNTS_I64, null = all) are sampled at the num_samples (a multiple of 64) arc-length fractions
 * k / (num_samples - 1) into samples f32[num_polylines, num_samples, 2], and the bounding box of every 64 consecutive samples
 * goes to group_boxes f32[num_polylines * num_samples / 64, 4] — what accv_polyline_sample_boxes writes for relative distances
 * = those fractions (polyline_common.cuh:58-163 semantics; finite samples and boxes bit for bit, NaN samples are NaN with an
 * unspecified sign bit), i.e. the input of
 * accv_draw_points_multiscale_f32 with ACCV_HM_GROUP_BOXES_GIVEN, which follows on the same stream. */
int accv_draw_heatmap_multiscale_sample_f32(float* const* heatmaps, const int* heights, const int* widths, const float* strides,
                                            int num_scales, int batch, const float* centers_xy, const float* boxes_xyxy,
                                            const void* counts, int max_num_targets, float diameter_to_sigma_factor,
                                            float k_scale, unsigned flags, const float* polylines_xy, int num_polylines,
                                            int points, const void* point_counts, int num_samples, float* samples,
                                            float* group_boxes, void* stream);

/* Lane raster of all scales in TWO launches (BASELINE config 3): sampled polyline points f32[batch, N, 2]
 * (source pixels; output of accv_polyline_sample, NaN = sample of an empty polyline) are drawn into every
 * heatmaps[s] f32[batch, heights[s], widths[s]] as Gaussians of `radius` around int(p / strides[s]) — for each scale the
 * result of accv_heatmap_targets_from_points_f32 + accv_draw_heatmap_batched_f32 with ACCV_HM_SMALL_RADII.  Launch 1
 * writes the bounding box of every 64 consecutive points into `workspace` (accv_draw_points_workspace_bytes); launch 2
 * covers the tiles of all (<= 4) scales and culls first by group box, then by point.  counts[b] (int32, or int64 with
 * ACCV_HM_COUNTS_I64) = number of leading points of sample b that are drawn.  Same map constraints as the multi-scale
 * box call.  The reference has no polyline rasteriser (polyline/functions.py:27-111 only samples). */
size_t accv_draw_points_workspace_bytes(int batch, int num_points);
int accv_draw_points_multiscale_f32(float* const* heatmaps, const int* heights, const int* widths, const float* strides,
                                    int num_scales, int batch, const float* points_xy, const void* counts, int num_points,
                                    int radius, float diameter_to_sigma_factor, float k_scale, unsigned flags,
                                    void* workspace, size_t workspace_bytes, void* stream);

/* Lane raster of all scales in ONE launch: the tile waves work from the polylines themselves — polylines_xy
 * f32[batch, lanes, points, 2] (source pixels), point_counts[batch * lanes] valid leading points per polyline (int32, or
 * int64 with ACCV_HM_POINT_COUNTS_I64; null = all), lane_counts[batch] valid leading polylines per frame (int32, or int64
 * with ACCV_HM_COUNTS_I64); every polyline is sampled at the num_samples arc-length fractions k / (num_samples - 1) (IEEE
 * float division; one sample at fraction 0 for num_samples == 1).  Result: bit for bit what accv_polyline_sample_boxes
 * (relative distances = those fractions, for every polyline) + accv_draw_points_multiscale_f32 write, without the sampler
 * launch, the sample buffer and the workspace: a wave tests the SEGMENTS of the frame's polylines against its tile and
 * repeats the sampler's arithmetic (polyline_common.cuh:58-163 semantics; csrc/polyline_arith.h) only for the stretch of
 * samples on segments in reach.  That work is repeated per tile and scale, so the launch saved pays for SPARSE lane sets
 * (one or two polylines per frame: 22.6-24.2 -> 17.8-18.6 us on config 3's maps) and the kernel takes only those:
 * accv_draw_polylines_fused_applicable(...) == 1 for 1..64 points per polyline, lanes x P2 <= 64 with P2 = points rounded
 * up to a power of two (>= 4), num_samples <= (points - 1) x P2 / 2, fine scales in the majority of the tiles; other shapes
 * return ACCV_EINVAL — use the two-launch composition for them.  Same map constraints as the calls above. */
#define ACCV_HM_POINT_COUNTS_I64 512u /* accv_draw_polylines_multiscale_f32: `point_counts` points to int64 */
int accv_draw_polylines_fused_applicable(const int* heights, const int* widths, int num_scales, int batch, int lanes,
                                         int points, int num_samples);
int accv_draw_polylines_multiscale_f32(float* const* heatmaps, const int* heights, const int* widths, const float* strides,
                                       int num_scales, int batch, const float* polylines_xy, int lanes, int points,
                                       const void* point_counts, const void* lane_counts, int num_samples, int radius,
                                       float diameter_to_sigma_factor, float k_scale, unsigned flags, void* stream);

/* Target-prep front end: float centres [n,2] (x,y) and boxes [n,4] (x0,y0,x1,y1) in source pixels ->
 * int32 centres [n,2] = int(c / stride) and radii [n] = max(1, int(ceil(min edge distance / stride))) in ONE kernel.
 * Semantics of get_centers_and_radii (packages/draw_heatmap/tests/_test_helpers.py:20-28; the DALI path uses
 * get_center_from_bboxes/get_radii_from_bboxes).  fp32 with IEEE division. */
int accv_heatmap_targets_from_boxes_f32(const float* centers_xy, const float* boxes_xyxy, long long num_objects,
                                        float stride, int32_t* out_centers, int32_t* out_radii, void* stream);

/* Lane front end (the "polyline raster" of BASELINE config 3): sampled polyline points f32[n,2] (x,y) in
 * source pixels (output of accv_polyline_sample) -> int32 centres [n,2] = int(p / stride) and radii [n] = `radius`;
 * NaN points (samples of empty polylines, polyline_kernels.cuh:216-245) get radius -1, which the splat never draws.
 * The reference has no rasteriser for polylines; this feeds its sampler's output to accv_draw_heatmap_batched_f32. */
int accv_heatmap_targets_from_points_f32(const float* points_xy, long long num_points, float stride, int radius,
                                         int32_t* out_centers, int32_t* out_radii, void* stream);

/* ------------------------------------------------------------------------------------------------ H2
 * Ragged-batch kernels (batching_helpers).  Shapes are given after flattening all batch dimensions to
 * `batch` and all trailing data dimensions to `row_bytes` (= elements per index * element size): the
 * indexed dimension sits between them.  COPY entry points are dtype-agnostic byte movers (bit-exact).
 * `indices` is [batch, idx_stride] of int32 (idx_i64 == 0) or int64; only the first `w_idx` slots of a
 * row are considered and of those only j < counts[i].  Negative indices wrap once; indices still out
 * of range are skipped and, if `err_counter` (device int*) is non-null, counted there (the reference
 * device-asserts: batched_indexing_access_cuda_impl.cu:79,143,185).  `counts` is int32 or int64.
 */

/* dst[i, j, :] = src[i, indices[i,j], :]   — forward of indexing_kernel
 * (batched_indexing_access_cuda_impl.cu:52-113, host batched_indexing_access_cuda.cpp:54-86).
 * src [batch, w_src, row], dst [batch, w_idx, row]; dst must be pre-filled by the caller. */
int accv_ragged_gather(const void* src, void* dst, const void* indices, const void* counts, long long batch,
                       long long w_src, long long w_idx, long long idx_stride, long long row_bytes, int idx_i64,
                       int counts_i64, int* err_counter, void* stream);

/* The same gather, but the kernel also writes the filler: dst[i, j, :] = `fill_bits` pattern (element of `elem_size`
 * in {1,2,4,8} bytes, little endian) for j >= counts[i] and for skipped out-of-range indices, so dst may be
 * uninitialised — one launch for torch::full + indexing_kernel of batched_indexing_access_cuda.cpp:82-85. */
int accv_ragged_gather_fill(const void* src, void* dst, const void* indices, const void* counts, long long batch,
                            long long w_src, long long w_idx, long long idx_stride, long long row_bytes,
                            uint64_t fill_bits, int elem_size, int idx_i64, int counts_i64, int* err_counter,
                            void* stream);

/* dst[i, indices[i,j], :] = src[i, j, :]   — overwrite direction of indexing_kernel (cpp:88-146 with
 * backward_accumulate == false).  src [batch, w_idx, row], dst [batch, w_dst, row]. */
int accv_ragged_scatter(const void* src, void* dst, const void* indices, const void* counts, long long batch,
                        long long w_idx, long long idx_stride, long long w_dst, long long row_bytes, int idx_i64,
                        int counts_i64, int* err_counter, void* stream);

/* dst[i, dst_indices[i,j], :] = src[i, src_indices[i,j], :] — map_values_by_index_pairs_kernel
 * (cu:115-160, cpp:170-200), overwrite mode. */
int accv_ragged_map_pairs(const void* src, void* dst, const void* src_indices, const void* dst_indices,
                          const void* counts, long long batch, long long w_src, long long w_idx, long long idx_stride,
                          long long w_dst, long long row_bytes, int idx_i64, int counts_i64, int* err_counter,
                          void* stream);

/* dst[i, indices[i,j], :] = const — insert_const_at_indices_kernel (cu:162-194; also builds bool masks,
 * cpp:202-228).  `elem_bits` holds the element's byte pattern (little endian) of `elem_size` in {1,2,4,8}. */
int accv_ragged_insert_const(void* dst, const void* indices, const void* counts, long long batch, long long w_idx,
                             long long idx_stride, long long w_dst, long long row_bytes, uint64_t elem_bits,
                             int elem_size, int idx_i64, int counts_i64, int* err_counter, void* stream);

/* data[i, j, :] = filler for j >= counts[i] — set_ragged_batch_padded_to_filler_value_kernel
 * (cu:196-213, cpp:230-245; CPU twin batched_indexing_access_cpu_impl.cpp:27-67). */
int accv_ragged_pad_fill(void* data, const void* counts, long long batch, long long width, long long row_bytes,
                         uint64_t elem_bits, int elem_size, int counts_i64, void* stream);

/* dst[i, dst_indices[i,j], k] += src[i, (src_indices ? src_indices[i,j] : j), k] with atomics — the
 * accumulate mode of indexing_kernel / map_values_by_index_pairs_kernel (cu:39-50, 103-108, 152-156); the
 * caller clears the touched slots first where "set first, then add" semantics are required.
 * acc_dtype: 0 f32, 1 f64, 2 i32, 3 i64, 4 f16, 5 bf16;  row_elems = elements per index. */
int accv_ragged_accumulate(const void* src, void* dst, const void* src_indices_or_null, const void* dst_indices,
                           const void* counts, long long batch, long long w_src, long long w_idx, long long idx_stride,
                           long long w_dst, long long row_elems, int acc_dtype, int idx_i64, int counts_i64,
                           int* err_counter, void* stream);

/* Ragged compaction front end (replaces the torch boolean indexing of batched_bool_indexing.py:195-221 and
 * batched_processing_py.py:245-268, 577-628): for every row the positions of non-zero mask bytes, in order,
 * as int64, zero-filled behind; out_sizes[i] = number of hits.  Only the first valid_counts[i] columns are
 * looked at when valid_counts is given.  out_indices is [batch, width]. */
int accv_ragged_mask_to_indices(const void* mask_u8, const void* valid_counts_or_null, int valid_i64, long long batch,
                                long long width, long long* out_indices, long long* out_sizes, void* stream);
/* The same with a caller-provided workspace of accv_ragged_mask_to_indices_workspace_bytes(batch, width) bytes (0 = not
 * needed): FEW, VERY WIDE rows (a dense anchor mask of a small batch) are cut into 4096-byte segments handled by one
 * workgroup each instead of one workgroup per row — in ONE launch for rows of up to 4 segments (every segment workgroup
 * counts its whole row itself; the workspace is not touched), in a count launch + a write launch through the workspace
 * beyond that.  Same results; without (enough) workspace the one-workgroup-per-row kernels run for the longer rows. */
size_t accv_ragged_mask_to_indices_workspace_bytes(long long batch, long long width);
int accv_ragged_mask_to_indices_ws(const void* mask_u8, const void* valid_counts_or_null, int valid_i64, long long batch,
                                   long long width, long long* out_indices, long long* out_sizes, void* workspace,
                                   size_t workspace_bytes, void* stream);


/* F3 — matched gather + element-wise loss + masked per-sample sum in ONE launch.  The caller pattern of
 * packages/batching_helpers/example/loss_computation.py:37-43 (batched_indexing_access of ground truth and prediction
 * through the two index lists of a matching) and :85-86 (sum_over_targets of the per-object loss):
 *   out[i] = sum_{j < counts[i]} w * sum_k l(a[i, idx_a[i,j], k] - b[i, idx_b[i,j], k]),  w = weights[i, idx_a[i,j]] or 1
 * kind: 0 = |d| (L1), 1 = d^2, 2 = smooth-L1 with `beta` (torch.nn.functional.smooth_l1_loss).  a f32[batch, w_a, row],
 * b f32[batch, w_b, row], indices [batch, idx_stride] int32/int64 (first w_idx slots), counts int32/int64, out f32[batch].
 * Deterministic (fixed-order tree reduction per sample).  Pairs with an out-of-range index contribute nothing. */
int accv_matched_pair_reduce_f32(const float* a, const float* b, const void* idx_a, const void* idx_b, const void* counts,
                                 const float* weights_or_null, long long batch, long long w_a, long long w_b,
                                 long long w_idx, long long idx_stride, long long row_elems, int kind, float beta,
                                 int idx_i64, int counts_i64, float* out, void* stream);
/* Its backward: grad_a[i, idx_a[i,j], k] += g[i] * w * l'(d), grad_b[...] -= the same, grad_w[i, idx_a[i,j]] += g[i] * l(d)
 * (float atomics; the gradient tensors must be zero-initialised by the caller; any of them may be NULL). */
int accv_matched_pair_reduce_bwd_f32(const float* a, const float* b, const void* idx_a, const void* idx_b,
                                     const void* counts, const float* weights_or_null, const float* grad_out,
                                     long long batch, long long w_a, long long w_b, long long w_idx,
                                     long long idx_stride, long long row_elems, int kind, float beta, int idx_i64,
                                     int counts_i64, float* grad_a_or_null, float* grad_b_or_null,
                                     float* grad_w_or_null, void* stream);

/* Round 3: the same two launches for every dtype the replaced gathers accept and for the reference example's own per-object
 * losses.  dtype: 0 f32, 1 f16, 2 bf16, 3 f64 — of a, b and weights; arithmetic, `out` and the gradient buffers are f32 (f64 for
 * f64 data).  kind 0-2 as above, plus
 *   3 = 1 - IoU of (x0, y0, x1, y1) boxes (row_elems == 4) with negative intersection extents clamped to 0 and the union
 *       clamped to `eps`: _per_object_bbox_overlap_loss, packages/batching_helpers/example/loss_computation.py:240-274;
 *       the backward follows torch's autograd of that code (clamps pass no gradient, max / min ties split it evenly);
 *   4 = L1 between one-hot class labels and scores: `a` holds INTEGER labels [batch, w_a] (int32, or int64 with
 *       ACCV_MP_LABELS_I64), b the scores [batch, w_b, row_elems]; sum_c |[c == label] - b[..., c]|
 *       (loss_computation.py:37-43 class branch, :225-238); a label outside [0, row_elems) matches no class.
 * flags: ACCV_MP_IDX_I64 / ACCV_MP_COUNTS_I64 / ACCV_MP_LABELS_I64. */
#define ACCV_MP_IDX_I64 1u
#define ACCV_MP_COUNTS_I64 2u
#define ACCV_MP_LABELS_I64 4u
int accv_matched_pair_reduce(const void* a, const void* b, const void* idx_a, const void* idx_b, const void* counts,
                             const void* weights_or_null, long long batch, long long w_a, long long w_b, long long w_idx,
                             long long idx_stride, long long row_elems, int kind, int dtype, float beta, float eps,
                             unsigned flags, void* out, void* stream);
int accv_matched_pair_reduce_bwd(const void* a, const void* b, const void* idx_a, const void* idx_b, const void* counts,
                                 const void* weights_or_null, const void* grad_out, long long batch, long long w_a,
                                 long long w_b, long long w_idx, long long idx_stride, long long row_elems, int kind,
                                 int dtype, float beta, float eps, unsigned flags, void* grad_a_or_null,
                                 void* grad_b_or_null, void* grad_w_or_null, void* stream);

/* Gaussian focal loss on a drawn heat-map target — the GaussianFocalLoss centerness term the draw_heatmap maps are drawn for
 * (packages/draw_heatmap/docs/intro.rst:7-25), forward and backward in one streaming pass each:
 *   p = clamp(sigmoid(logits), eps, 1 - eps)   (clamp_eps = 0: no clamp)
 *   l = pos_weight * [target == 1] * -log(p + 1e-12) * (1 - p)^alpha
 *     + neg_weight * -log(1 - p + 1e-12) * p^alpha * (1 - target)^gamma
 *   out_loss = sum(l) / denom,  denom = max(#{target == 1}, 1) (ACCV_FL_AVG_NUM_POS, counted exactly in the same pass),
 *              avg_factor (ACCV_FL_AVG_VALUE) or *avg_factor_dev (ACCV_FL_AVG_DEVICE, f32 device scalar)
 * logits [numel] of dtype 0 f32, 1 f16, 2 bf16 (the codes of accv_matched_pair_reduce), target f32 [numel]; arithmetic in
 * f32, per-block partials in f64 summed in a fixed order by a second one-block launch: no atomics, bitwise reproducible.
 * out_loss and out_denom are f32 device scalars; the backward reads out_denom.  alpha >= 1, gamma >= 0, 0 <= clamp_eps < 0.5.
 * workspace: accv_gaussian_focal_loss_workspace_bytes(numel) bytes of device memory, 16-byte aligned.  numel == 0 launches
 * nothing (and writes nothing). */
#define ACCV_FL_AVG_NUM_POS 0
#define ACCV_FL_AVG_VALUE 1
#define ACCV_FL_AVG_DEVICE 2
size_t accv_gaussian_focal_loss_workspace_bytes(long long numel);
int accv_gaussian_focal_loss(const void* logits, const float* target, long long numel, int dtype, float alpha, float gamma,
                             float pos_weight, float neg_weight, float clamp_eps, int avg_mode, float avg_factor,
                             const float* avg_factor_dev, float* out_loss, float* out_denom, void* workspace,
                             size_t workspace_bytes, void* stream);
/* Its backward, element-wise: grad_logits = *grad_out / *denom * dl/dlogits in the logits dtype, written once (no atomics, no
 * zero-initialisation needed).  The clamp passes gradient only where eps <= sigmoid(x) <= 1 - eps (torch.clamp's inclusive
 * mask); the rest is torch autograd of the formula above. */
int accv_gaussian_focal_loss_bwd(const void* logits, const float* target, long long numel, int dtype, float alpha, float gamma,
                                 float pos_weight, float neg_weight, float clamp_eps, const float* grad_out,
                                 const float* denom, void* grad_logits, void* stream);

/* Heat-map peak extraction — mmdet's get_local_maximum + get_topk_from_heatmap (models/utils/gaussian_target.py), the
 * read-back half of the maps draw_heatmap draws, fused into two launches:
 *   s = x * (x == max over the kernel x kernel window)   (window clipped at the border: max_pool2d's -inf padding)
 *   per group the k largest s in descending order, equal scores by ascending flat index in the group
 *   (= torch.sort(s, descending=True, stable=True)[:k]).  A group is a frame of C*H*W elements (per_class == 0) or one
 *   (b, c) plane of H*W (per_class != 0); it must hold at least k and fewer than 2^32 - 1 elements.
 * x [B, C, H, W] contiguous, dtype 0 f32, 1 f16, 2 bf16 (the codes of accv_gaussian_focal_loss); kernel odd in 1..7;
 * 1 <= k <= 1024.  Outputs [groups, k]: scores in the input dtype (the values of x, suppressed ones +0.0), indices
 * y * W + x in the plane, classes (the plane's channel), ys, xs — all int64.  No atomics decide the order: results are
 * bitwise reproducible.  workspace: accv_heatmap_peaks_workspace_bytes(B, C, H, W, k) bytes of device memory, 16-byte
 * aligned (0 for sizes the call refuses).  Returns ACCV_EINVAL (negative size, unknown dtype, even or out-of-range kernel,
 * k out of range or above the group size, a group of 2^32 - 1 or more elements, null pointers) or ACCV_EWORKSPACE before
 * touching the device, ACCV_ELAUNCH if a launch fails; B == 0 launches nothing. */
size_t accv_heatmap_peaks_workspace_bytes(long long B, long long C, long long H, long long W, int k);
int accv_heatmap_peaks(const void* x, int dtype, long long B, long long C, long long H, long long W, int kernel, int k,
                       int per_class, void* scores, long long* indices, long long* classes, long long* ys, long long* xs,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------ centre-point regression
 * The regression branch of a centre-point head (CenterNet / CenterPoint: offset, size, height, rot, vel at the object
 * centres) without the cat / permute / gather / scatter passes over the maps of mmdet's transpose_and_gather_feat.
 *
 * Maps: a HOST array `maps` of num_maps (1..ACCV_CR_MAX_MAPS) device pointers and a HOST array `channels` of their
 * channel counts C_i >= 0; map i is [B, C_i, H, W] contiguous of dtype 0 f32, 1 f16, 2 bf16 (the codes of
 * accv_gaussian_focal_loss), element-aligned.  Their channels are concatenated in the order given,
 * C = sum C_i <= ACCV_CR_MAX_CHANNELS; H * W < 2^31; element offsets are 64-bit.
 * Centres: int32 [B, N, 2] as (x, y) with `counts` [B] (int32, int64 with ACCV_CR_COUNTS_I64; clamped to [0, N]), or with
 * ACCV_CR_INDEX_FORM int64 [B, N] in-plane indices y * W + x (counts is not read, every slot counts).  A slot is valid
 * when it lies below its frame's count and its cell inside the map; nothing outside the maps is ever read.
 * Every entry returns ACCV_EINVAL (negative size, unknown dtype / kind / flag / avg mode, more than ACCV_CR_MAX_MAPS maps
 * or ACCV_CR_MAX_CHANNELS channels, H * W >= 2^31, null or misaligned pointers, null params) or ACCV_EWORKSPACE before
 * touching the device, ACCV_ELAUNCH if a launch fails.  No atomics, no host synchronisation, bitwise reproducible. */
#define ACCV_CR_MAX_MAPS 8
#define ACCV_CR_MAX_CHANNELS 64
#define ACCV_CR_COUNTS_I64 1u
#define ACCV_CR_INDEX_FORM 2u
#define ACCV_CR_WEIGHTS_PER_CHANNEL 4u /* weights are [B, N, C] instead of [B, N] */
#define ACCV_CR_L1 0                   /* the kind codes of accv_matched_pair_reduce */
#define ACCV_CR_SMOOTH_L1 2
/* the scalar parameters of the loss, host memory, read during the call (by pointer so the entries take integers only) */
typedef struct accv_center_regression_params {
    int kind;         /* ACCV_CR_L1 or ACCV_CR_SMOOTH_L1 */
    int avg_mode;     /* ACCV_FL_AVG_NUM_POS (max(number of valid slots, 1)), ACCV_FL_AVG_VALUE, ACCV_FL_AVG_DEVICE */
    float beta;       /* smooth-L1 transition point, > 0 */
    float avg_factor; /* the denominator of ACCV_FL_AVG_VALUE */
} accv_center_regression_params;
/* out[b, n, c] (contiguous [B, N, C], the maps' dtype) = maps[b, c, y, x] bit for bit at a valid slot, +0 elsewhere.
 * One launch; B * N * C == 0 launches nothing. */
int accv_gather_at_centers(const void* const* maps, const int* channels, int num_maps, int dtype, long long B, long long H,
                           long long W, const void* centers, const void* counts, long long N, unsigned flags, void* out,
                           void* stream);
/* Its backward: writes every element of every gradient map exactly once — +0, and at each valid cell the sum over the
 * frame's valid slots on that cell, in ascending slot order, of grad_rows[b, n, c] ([B, N, C] contiguous, the maps'
 * dtype), accumulated in f32 and rounded once.  The gradient maps need no initialisation.  One launch; B == 0 launches
 * nothing, N == 0 writes zeros. */
int accv_scatter_at_centers(void* const* grad_maps, const int* channels, int num_maps, int dtype, long long B, long long H,
                            long long W, const void* centers, const void* counts, long long N, unsigned flags,
                            const void* grad_rows, void* stream);
/* *out_loss = sum over valid (b, n) and c of w * l(maps[b, c, y, x] - targets[b, n, c]) / denom, *out_denom = denom (f32
 * device scalars).  l is L1 or smooth-L1(beta) with torch's definitions; targets f32 [B, N, C]; weights NULL (1), f32
 * [B, N] or, with ACCV_CR_WEIGHTS_PER_CHANNEL, [B, N, C]; rows of invalid slots are never read.  Arithmetic in f32
 * (f16 / bf16 widened exactly), one f64 partial per frame, added in a fixed order by a second one-block launch.
 * avg_factor_dev: the f32 device scalar of ACCV_FL_AVG_DEVICE.  ACCV_CR_INDEX_FORM is not taken.
 * workspace: accv_center_regression_loss_workspace_bytes(B) bytes of device memory, 16-byte aligned.  B == 0 launches
 * nothing (and writes nothing). */
size_t accv_center_regression_loss_workspace_bytes(long long B);
int accv_center_regression_loss(const void* const* maps, const int* channels, int num_maps, int dtype, long long B,
                                long long H, long long W, const void* centers, const void* counts, long long N,
                                unsigned flags, const float* targets, const float* weights_or_null,
                                const accv_center_regression_params* params, const float* avg_factor_dev, float* out_loss,
                                float* out_denom, void* workspace, size_t workspace_bytes, void* stream);
/* Its backward, with the complete-write contract of accv_scatter_at_centers: the contribution of slot n to channel c of
 * its cell is (w * dl/dd) * (*grad_out / *denom), evaluated in f32 in exactly this order; contributions to one cell add
 * in ascending slot order in f32 and are rounded once to the maps' dtype.  grad_out and denom are f32 device scalars
 * (denom: out_denom of the forward).  params->avg_mode and avg_factor are not read. */
int accv_center_regression_loss_bwd(const void* const* maps, void* const* grad_maps, const int* channels, int num_maps,
                                    int dtype, long long B, long long H, long long W, const void* centers,
                                    const void* counts, long long N, unsigned flags, const float* targets,
                                    const float* weights_or_null, const accv_center_regression_params* params,
                                    const float* grad_out, const float* denom, void* stream);

/* ------------------------------------------------------------------------------------------------ centre-point targets
 * The target side of a centre-point head (mmdet3d's CenterHead.get_targets_single) for a ragged batch of 3D boxes and
 * every task of the head in ONE launch: integer centres, Gaussian radii, in-task labels, regression targets, in-plane
 * indices and the source slot of every kept object, compacted per (task, frame) in ascending slot order.
 *
 * boxes: f32 [B, N, D] contiguous, D = 7 or 9 as (x, y, z, dx, dy, dz, yaw[, vx, vy]); labels [B, N] int32 (int64 with
 * ACCV_CT_LABELS_I64); counts [B] int32 (int64 with ACCV_CT_COUNTS_I64), clamped to [0, N]: only slots below it are read.
 * params->class_task[c] is the task of class c (ACCV_CT_NO_TASK: none) and class_pos[c] its position inside that task; a
 * label outside [0, ACCV_CT_MAX_CLASSES) belongs to no task.  Per frame b and task t, in float32 (the operation sequence
 * is written out in csrc/center_targets_arith.h: correctly rounded division (__fdiv_rn) and square root (sqrtf under
 * hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt), nothing contracted):
 *   candidates  the slots n < counts[b] whose label is in task t, ascending; only the first max_objs of them go on
 *   kept        w = dx / vs0 / f > 0, l = dy / vs1 / f > 0, cx = (x - pc0) / vs0 / f in (-1, W), cy likewise in (-1, H);
 *               NaN fails; cell = ((int)cx, (int)cy), truncated toward zero
 *   radius      max(min_radius, (int)gaussian_radius((l, w), gaussian_overlap)) (CenterPoint's three-root rule; a NaN
 *               root converts to 0, the conversion saturates)
 *   target      (cx - cell_x, cy - cell_y, z, dims, sin yaw, cos yaw[, vx, vy]), D + 1 channels; dims = log(dx, dy, dz)
 *               with norm_bbox, else raw
 * Outputs, [T, B, M, ...] contiguous with M >= min(max_objs, N): centers int32 (x, y), radii int32, out_labels int32,
 * targets f32 [.., D + 1], indices int64 (y * W + x), source int32 (the slot n), out_sizes int64 [T, B] (kept count).
 * Slots kept .. M-1 are written too: 0 everywhere, source -1 (a complete write).  One workgroup per (frame, task), no
 * atomics, no host synchronisation, bitwise reproducible.  B == 0 or M == 0 launches nothing and writes nothing.
 * Returns ACCV_EINVAL (null params, negative size, T outside 1..ACCV_CT_MAX_TASKS, D not 7 / 9, unknown flags, a class of
 * task >= T, non-positive voxel size / out_size_factor, W or H < 1 or W * H >= 2^31, N above 2^31 - 1, M below
 * min(max_objs, N), null or misaligned pointers) before touching the device, ACCV_ELAUNCH if the launch fails.
 * accv_center_point_targets_host runs the same operation sequence serially on host memory. */
#define ACCV_CT_MAX_TASKS 8
#define ACCV_CT_MAX_CLASSES 64
#define ACCV_CT_NO_TASK 255
#define ACCV_CT_LABELS_I64 1u
#define ACCV_CT_COUNTS_I64 2u
/* the scalar parameters and the class table, host memory, read during the call */
typedef struct accv_center_point_targets_params {
    double pc_range[2];        /* x, y of the range's lower corner */
    double voxel_size[2];      /* x, y; > 0 */
    double out_size_factor;    /* > 0 */
    double gaussian_overlap;
    int min_radius;
    int max_objs;              /* >= 0 */
    int norm_bbox;
    int num_tasks;             /* T */
    unsigned char class_task[ACCV_CT_MAX_CLASSES];
    unsigned char class_pos[ACCV_CT_MAX_CLASSES];
} accv_center_point_targets_params;
int accv_center_point_targets(const float* boxes, const void* labels, const void* counts, unsigned flags, long long B,
                              long long N, long long D, long long W, long long H, long long M,
                              const accv_center_point_targets_params* params, int* centers, int* radii, int* out_labels,
                              float* targets, long long* indices, int* source, long long* out_sizes, void* stream);
int accv_center_point_targets_host(const float* boxes, const void* labels, const void* counts, unsigned flags, long long B,
                                   long long N, long long D, long long W, long long H, long long M,
                                   const accv_center_point_targets_params* params, int* centers, int* radii,
                                   int* out_labels, float* targets, long long* indices, int* source, long long* out_sizes);

/* --------------------------------------------------------------------------------- BEV box augmentation + range filter
 * What the raw 3D boxes of a sample go through before accv_center_point_targets, for a ragged batch in ONE launch: the
 * reference's BEVBBoxesTransformer3D (packages/dali_pipeline_framework/.../processing_steps/bev_bboxes_transformer_3d.py:
 * a global rotation about z, then a uniform scaling, then a translation of centres, sizes, yaws and velocities, and the
 * update of every matrix that maps to or from the augmented frame), PointsInRangeCheck on the centres
 * (processing_steps/points_in_range_check.py; check_points_in_box of operators_impl/numba_operators) and the
 * ConditionalElementRemover over the resulting is_active flag; wired at examples/pipeline_setup/stream_petr_pipeline.py:409-497.
 *
 * boxes: f32 [B, N, D] contiguous, D = 7 or 9 as (x, y, z, dx, dy, dz, yaw[, vx, vy]); rows: f32 [B, 7], the frame's
 * (angle, cos, sin, scale, tx, ty, tz), the cosine and sine read as given; labels: null or [B, N] int32 (int64 with
 * ACCV_BA_LABELS_I64); valid: null or bool bytes [B, N], the rest of the keep condition; counts [B] int32 (int64 with
 * ACCV_BA_COUNTS_I64), clamped to [0, N]: only slots below it are read.  A slot is kept iff valid and, with
 * params->has_range, range_min <= centre <= range_max on all three coordinates (the float32 centre against the float64
 * borders as the reference compares them, both inclusive, NaN fails, +-inf allowed), tested on the raw centre or, with
 * ACCV_BA_RANGE_ON_OUTPUT, on the augmented one.
 * The float32 operation sequence is written out in csrc/bev_augment_arith.h (nothing contracted, division correctly
 * rounded).  params->point_in[i]: f32 [B, point_count[i], point_rows[i] = 3 or 4, 4], matrices applied to points of the
 * augmented frame, M . A^-1 written to point_out[i]; params->frame_in[i]: f32 [B, frame_count[i], 4, 4], matrices whose
 * results are points of that frame, A . M written to frame_out[i]; A = T . S . R.  Inputs and outputs do not overlap.
 * Outputs: out_boxes f32 [B, N, D], the kept boxes augmented and compacted in ascending slot order; out_labels [B, N] of
 * the labels' type (null without labels); source int32 [B, N], the input slot; keep bool bytes [B, N] over the INPUT
 * slots; out_sizes int64 [B], the kept count.  Slots kept .. N-1 are written too: 0 everywhere, source -1, and keep is 0
 * from counts[b] on (a complete write).  One workgroup per frame, no atomics, no workspace, no host synchronisation,
 * bitwise reproducible and bit-equal to accv_bev_augment_host, which runs the same operation sequence serially on host
 * memory.  B == 0 launches nothing and writes nothing.  Returns ACCV_EINVAL (null params, negative size, D not 7 / 9,
 * unknown flags, more transforms than the maxima, matrices of other than 3 or 4 rows, N above 2^31 - 1, null or misaligned
 * pointers, labels without out_labels) before touching the device, ACCV_ELAUNCH if the launch fails. */
#define ACCV_BA_MAX_POINT_TRANSFORMS 4
#define ACCV_BA_MAX_FRAME_TRANSFORMS 2
#define ACCV_BA_COUNTS_I64 1u
#define ACCV_BA_LABELS_I64 2u
#define ACCV_BA_RANGE_ON_OUTPUT 4u
/* the range and the matrix tensors, host memory, read during the call */
typedef struct accv_bev_augment_params {
    double range_min[3], range_max[3];   /* used with has_range */
    const float* point_in[ACCV_BA_MAX_POINT_TRANSFORMS];
    float* point_out[ACCV_BA_MAX_POINT_TRANSFORMS];
    long long point_count[ACCV_BA_MAX_POINT_TRANSFORMS];   /* K, matrices per frame */
    const float* frame_in[ACCV_BA_MAX_FRAME_TRANSFORMS];
    float* frame_out[ACCV_BA_MAX_FRAME_TRANSFORMS];
    long long frame_count[ACCV_BA_MAX_FRAME_TRANSFORMS];   /* K, matrices per frame */
    int point_rows[ACCV_BA_MAX_POINT_TRANSFORMS];          /* R = 3 or 4 */
    int num_point_transforms;
    int num_frame_transforms;
    int has_range;
} accv_bev_augment_params;
int accv_bev_augment(const float* boxes, const float* rows, const void* labels, const unsigned char* valid, const void* counts,
                     unsigned flags, long long B, long long N, long long D, const accv_bev_augment_params* params,
                     float* out_boxes, void* out_labels, int* source, unsigned char* keep, long long* out_sizes, void* stream);
int accv_bev_augment_host(const float* boxes, const float* rows, const void* labels, const unsigned char* valid,
                          const void* counts, unsigned flags, long long B, long long N, long long D,
                          const accv_bev_augment_params* params, float* out_boxes, void* out_labels, int* source,
                          unsigned char* keep, long long* out_sizes);

/* ------------------------------------------------------------------------------------------------ visible-box selection
 * Which 2D boxes of a camera image are drawn at all: the occlusion test and the minimum-size test of the reference's
 * VisibleBboxSelector step (packages/dali_pipeline_framework/.../processing_steps/visible_bbox_selector.py; the operators
 * check_bbox_visibiity / check_minimum_bbox_size, operators_impl/numba_operators/numba_operators.py:240-403; wired at
 * examples/pipeline_setup/stream_petr_pipeline.py:397-452) for a ragged batch in ONE launch and without the reference's
 * H x W canvas.
 *
 * boxes: f32 [B, G, 4] contiguous, rows (x1, y1, x2, y2) with the corners in either order; depths: f32 [B, G], smaller is
 * nearer, needed with check_occlusion; counts [B] int32 (int64 with ACCV_VB_COUNTS_I64), clamped to [0, G]: only slots
 * below it are read.  image_hw: null (every frame is params->image_h x image_w) or [B, 2] int32 (int64 with
 * ACCV_VB_HW_I64) rows (H, W), read where the boxes are; either way H and W are clamped to [0, 2^24].  Per frame, in
 * float32 (written out in csrc/visible_boxes_arith.h):
 *   painted     corners ordered, lower edges floor and upper edges ceil (ceil and floor with shrink_to_int), each rounded
 *               edge clamped to [-1, W + 1] / [-1, H + 1]; a box with lo_x > W, hi_x < 0, lo_y > H, hi_y < 0 or a NaN
 *               coordinate paints nothing; the rest paints its clip to the image, the half-open [x0, x1) x [y0, y1)
 *   order       np.argsort(-depth, kind="stable"), last painted on top: j above i iff depth_j < depth_i, or equal and
 *               j > i; -0.0 == 0.0; a NaN depth lies above every number, two NaNs tie
 *   occlusion   true iff some pixel of the painted rectangle is in the painted rectangle of no box above
 *   size        raw coordinates clipped to [0, W] / [0, H]; |x2 - x1| >= (float)minimum_size and |y2 - y1| likewise (NaN
 *               fails); a box that fails still occludes
 * out: bool bytes [B, G], the AND of the requested checks, 0 in the slots from counts[b] on: every byte is written.  One
 * workgroup per frame, memory independent of H and W, no atomics, no host synchronisation, bitwise reproducible.  B == 0 or
 * G == 0 launches nothing.  Returns ACCV_EINVAL (null params, negative size, unknown flags, neither check requested,
 * G > ACCV_VB_MAX_BOXES, null or misaligned pointers, occlusion without depths) before touching the device, ACCV_ELAUNCH if
 * the launch fails.  accv_visible_boxes_host runs the same integer algorithm serially on host memory. */
#define ACCV_VB_MAX_BOXES 256
#define ACCV_VB_COUNTS_I64 1u
#define ACCV_VB_HW_I64 2u
typedef struct accv_visible_boxes_params {
    double minimum_size;       /* used with check_size */
    long long image_h, image_w; /* used when image_hw is null */
    int check_occlusion;
    int check_size;
    int shrink_to_int;
} accv_visible_boxes_params;
int accv_visible_boxes(const float* boxes, const float* depths, const void* counts, const void* image_hw, unsigned flags,
                       long long B, long long G, const accv_visible_boxes_params* params, unsigned char* out, void* stream);
int accv_visible_boxes_host(const float* boxes, const float* depths, const void* counts, const void* image_hw,
                            unsigned flags, long long B, long long G, const accv_visible_boxes_params* params,
                            unsigned char* out);

/* -------------------------------------------------------------------------------------------- camera-box augmentation
 * The annotation side of the reference's camera pipeline for a ragged batch in ONE launch: what AffineTransformer does to
 * its point fields and projection matrices with the 2 x 3 matrix that warps the image (processing_steps/
 * affine_transformer.py), then VisibleBboxSelector, the condition "categories >= 0 and is_visible", the
 * ConditionalElementRemover over bboxes, centers, depths and categories, and the two CoordinateCroppers; wired at
 * examples/pipeline_setup/stream_petr_pipeline.py (pre_processing_steps).  A frame is one camera image.
 *
 * boxes: f32 [F, G, 4] contiguous, rows (x1, y1, x2, y2), corners in either order; transforms: f32 [F, 2, 3], the forward
 * matrix [[a, b, tx], [c, d, ty]] accv_prepare_images takes; centers: null or f32 [F, G, 2]; depths: null or f32 [F, G],
 * needed with check_occlusion; categories: null or [F, G] int32 (int64 with ACCV_CB_CATEGORIES_I64); valid: null or bool
 * bytes [F, G]; counts [F] int32 (int64 with ACCV_CB_COUNTS_I64), clamped to [0, G]: only slots below it are read.  The
 * image extent is params->image_h x image_w for every frame or, with params->image_hw, rows (H, W) of an [F, 2] int32
 * (int64 with ACCV_CB_HW_I64) tensor read where the boxes are; either way clamped to [0, 2^24].  Per frame, in float32 (the
 * operation sequence is written out in csrc/camera_boxes_arith.h, nothing contracted):
 *   warp        every corner and the centre become ((a*x + b*y) + tx, (c*x + d*y) + ty); with order_corners the box is
 *               rewritten as (min_x, min_y, max_x, max_y) by the `<` selection of the visible-box selection
 *   matrices    params->mat_in[i]: f32 [F, mat_count[i], mat_rows[i], mat_cols[i]] with 3 or 4 rows and columns; row 0
 *               becomes (a*m0j + b*m1j) + tx*m2j, row 1 (c*m0j + d*m1j) + ty*m2j, rows 2 and 3 are copied bit for bit, to
 *               mat_out[i]
 *   visible     the decision of accv_visible_boxes on the warped boxes before any crop (check_occlusion, check_size with
 *               minimum_size, shrink_to_int); with neither check every real slot is visible
 *   keep        visible && category >= 0 (with categories) && valid (with valid); a box that is not kept still occludes
 *   crop        with params->crop every kept coordinate v becomes v < 0 ? 0 : (v > E ? E : v), E = W for x, H for y
 * Outputs: out_boxes f32 [F, G, 4], out_centers f32 [F, G, 2], out_depths f32 [F, G], out_categories [F, G] of the
 * categories' type (each null exactly when its input is null), source int32 [F, G]: the kept slots compacted in ascending
 * slot order, the rest of each row 0 and source -1; keep and visible bool bytes [F, G] over the INPUT slots, 0 from
 * counts[f] on; out_sizes int64 [F], the kept count.  Every output element is written exactly once; inputs and outputs do
 * not overlap.  One workgroup per frame, no atomics, no workspace, no host synchronisation, bitwise reproducible and
 * bit-equal to accv_camera_boxes_host, which runs the same operation sequence serially on host memory.  F == 0, or G == 0
 * without a matrix element, launches nothing and writes nothing; G == 0 with matrices writes them and out_sizes.  Returns ACCV_EINVAL (null params, negative size, unknown flags,
 * G > ACCV_CB_MAX_BOXES, more than ACCV_CB_MAX_MATRICES matrix tensors, matrices of other than 3 or 4 rows or columns, null or
 * misaligned pointers, occlusion without depths, an input without its output or the reverse, more workgroups than a grid
 * holds) before touching the device, ACCV_ELAUNCH if the launch fails. */
#define ACCV_CB_MAX_BOXES 256
#define ACCV_CB_MAX_MATRICES 4
#define ACCV_CB_COUNTS_I64 1u
#define ACCV_CB_HW_I64 2u
#define ACCV_CB_CATEGORIES_I64 4u
/* the scalar parameters, the image extent and the matrix tensors; host memory, read during the call */
typedef struct accv_camera_boxes_params {
    double minimum_size;        /* used with check_size */
    long long image_h, image_w; /* used when image_hw is null */
    const void* image_hw;       /* null or [F, 2] where the boxes are */
    const float* mat_in[ACCV_CB_MAX_MATRICES];
    float* mat_out[ACCV_CB_MAX_MATRICES];
    long long mat_count[ACCV_CB_MAX_MATRICES];   /* K, matrices per frame */
    int mat_rows[ACCV_CB_MAX_MATRICES];          /* 3 or 4 */
    int mat_cols[ACCV_CB_MAX_MATRICES];          /* 3 or 4 */
    int num_matrices;
    int check_occlusion;
    int check_size;
    int shrink_to_int;
    int crop;
    int order_corners;
} accv_camera_boxes_params;
int accv_camera_boxes(const float* boxes, const float* transforms, const float* centers, const float* depths,
                      const void* categories, const unsigned char* valid, const void* counts, unsigned flags, long long F,
                      long long G, const accv_camera_boxes_params* params, float* out_boxes, float* out_centers,
                      float* out_depths, void* out_categories, int* source, unsigned char* keep, unsigned char* visible,
                      long long* out_sizes, void* stream);
int accv_camera_boxes_host(const float* boxes, const float* transforms, const float* centers, const float* depths,
                           const void* categories, const unsigned char* valid, const void* counts, unsigned flags,
                           long long F, long long G, const accv_camera_boxes_params* params, float* out_boxes,
                           float* out_centers, float* out_depths, void* out_categories, int* source, unsigned char* keep,
                           unsigned char* visible, long long* out_sizes);

/* ------------------------------------------------------------------------------------------- box-to-heat-map targets
 * The step after the visible-box selection: the reference's BoundingBoxToHeatmapConverter
 * (packages/dali_pipeline_framework/.../processing_steps/bounding_box_to_heatmap_converter.py; its helpers
 * apply_clipping_and_get_with_clipping_info / get_is_active, operators_impl/python_operator_functions/
 * python_operator_functions.py:103-252, get_center_from_bboxes / get_radii_from_bboxes, operators_impl/numba_operators/
 * numba_operators.py:788-905, and the native rasteriser ext_impl/DrawGaussians.cc:32-76) for a ragged batch in ONE launch:
 * the Gaussian maps and the per-object side outputs a CenterNet-style head trains on.
 *
 * boxes: f32 [B, G, 4] contiguous, rows (x1, y1, x2, y2) in image pixels, corners in either order on either diagonal;
 * centers: f32 [B, G, 2] or null (the box centre); categories: [B, G] int32 (int64 with ACCV_BH_CATEGORIES_I64), needed when
 * params->num_categories > 0; is_valid: bool bytes [B, G] or null; counts [B] int32 (int64 with ACCV_BH_COUNTS_I64), clamped
 * to [0, G]: only slots below it are read.  image_hw: null (every frame is params->image_h x image_w) or [B, 2] int32
 * (int64 with ACCV_BH_HW_I64) rows (H, W), read where the boxes are; either way clamped to [0, 2^24].  Per object, in float32
 * (the operation sequence is written out in csrc/box_heatmap_arith.h):
 *   scaling     sx = (float)map_w / (float)W, sy = (float)map_h / (float)H; box and centre coordinates times sx / sy; an
 *               object with a scaled coordinate that is not finite is inactive and all its outputs are 0
 *   clipping    each scaled coordinate to [0, map_w - 1] / [0, map_h - 1]: bboxes_heatmap (input corner order) and the
 *               clipped centre; height_width = (|y2 - y1|, |x2 - x1|) of the clipped box
 *   centre      center = floor(clipped centre) as (x, y), center_offset = clipped - floor
 *   radius      min of the four distances from the clipped centre to the clipped box's edges, max(0, .), times
 *               radius_scaling_factor, clamped to [max(0.5, min_radius), max_radius]
 *   is_active   finite && (h * w) / (unclipped scaled h * w) >= min_fraction_area_clipping && the size test (h >= min_h &&
 *               w >= min_w, global or of the object's category) && 0 <= category < num_categories (when num_categories
 *               > 0) && is_valid; NaN fails every comparison
 *   drawing     R = (int)ceil(radius), sigma = radius * radius_to_sigma_factor; an active object writes
 *               k_for_classes[plane] * exp(-(dx^2 + dy^2) / (2 sigma^2)) to the pixels of [cx - R, cx + R] x [cy - R, cy + R]
 *               inside the map, on plane `category` (plane 0 without per_category_heatmap), combined by max with 0 and
 *               with the other objects
 * heatmap: f32 [B, planes, map_h, map_w], planes = num_categories with per_category_heatmap, else 1; every element is
 * written, nothing is read or cleared beforehand.  Per-object outputs [B, G, ...]: is_active bool bytes, center int32 (x, y),
 * center_offset f32 (x, y), height_width f32 (h, w), bboxes_heatmap f32 [.., 4], radii f32; slots from counts[b] on are
 * written as 0.  One workgroup per (frame, plane, ACCV_BH_TILE_W x ACCV_BH_TILE_H tile), no atomics, no workspace, no host
 * synchronisation, bitwise reproducible.  B == 0 launches nothing; G == 0 still writes the (zero) maps.  Returns ACCV_EINVAL
 * (null params, negative size, unknown flags, G > ACCV_BH_MAX_BOXES, num_categories outside 0..ACCV_BH_MAX_CATEGORIES, both
 * minimum-size forms at once, per-category maps or sizes without categories, a map extent outside [1, 2^24], a scalar that
 * is not finite, max_radius outside (0, 16384], radius_to_sigma_factor <= 0, null or misaligned pointers, more workgroups
 * than a grid holds) before touching the device, ACCV_ELAUNCH if the launch fails.  accv_box_heatmap_host runs the same
 * per-object operation sequence serially on host memory and paints with std::exp. */
#define ACCV_BH_MAX_BOXES 256
#define ACCV_BH_MAX_CATEGORIES 128
#define ACCV_BH_TILE_W 64
#define ACCV_BH_TILE_H 16
#define ACCV_BH_COUNTS_I64 1u
#define ACCV_BH_HW_I64 2u
#define ACCV_BH_CATEGORIES_I64 4u
/* the scalar parameters and the per-category tables, host memory, read during the call (they travel to the kernel by value) */
typedef struct accv_box_heatmap_params {
    long long image_h, image_w;             /* used when image_hw is null */
    long long map_h, map_w;
    double min_fraction_area_clipping;
    double min_radius, max_radius;
    double radius_scaling_factor;
    double radius_to_sigma_factor;
    double min_object_size[2];              /* (h, w), used with has_min_object_size */
    int num_categories;                     /* 0: categories are not used */
    int per_category_heatmap;
    int has_min_object_size;
    int has_per_category_min_object_sizes;
    float per_category_min_object_sizes[ACCV_BH_MAX_CATEGORIES][2];   /* (h, w) per category */
    float k_for_classes[ACCV_BH_MAX_CATEGORIES];                      /* per plane */
} accv_box_heatmap_params;
int accv_box_heatmap(const float* boxes, const float* centers, const void* categories, const unsigned char* is_valid,
                     const void* counts, const void* image_hw, unsigned flags, long long B, long long G,
                     const accv_box_heatmap_params* params, float* heatmap, unsigned char* is_active, int* center,
                     float* center_offset, float* height_width, float* bboxes_heatmap, float* radii, void* stream);
int accv_box_heatmap_host(const float* boxes, const float* centers, const void* categories, const unsigned char* is_valid,
                          const void* counts, const void* image_hw, unsigned flags, long long B, long long G,
                          const accv_box_heatmap_params* params, float* heatmap, unsigned char* is_active, int* center,
                          float* center_offset, float* height_width, float* bboxes_heatmap, float* radii);

/* ------------------------------------------------------------------------------------------ camera-image preparation
 * The image side of the reference's camera pipeline (packages/dali_pipeline_framework/.../processing_steps/: AffineTransformer
 * through fn.warp_affine with bilinear interpolation and fill 0, PhotoMetricDistorter._process_images,
 * ImageToTileSizePadder, ImageMeanStdDevNormalizer / ImageRange01Normalizer; four DALI operators and four passes there) for a
 * batch of decoded images in ONE launch: the uint8 source is read where it is sampled, the float result is written once.
 *
 * images: u8 [batch, source_h, source_w, 3] contiguous.  source_hw: null or [batch, 2] int32 (int64 with
 * params->source_hw_i64) rows (H, W), read where the images are and clamped to [0, source_h] x [0, source_w]: the valid region
 * of each image; bytes outside it are never read and count as outside the image.  transforms: null or f32 [batch, 2, 3],
 * the FORWARD map [[a, b, tx], [c, d, ty]] from source to output coordinates (pixel i covers [i, i + 1), its centre is at
 * i + 0.5); null takes source pixel (X, Y) as is and needs output = source extent.  photometric: null or f32 [batch, 6] rows
 * (delta, alpha_pre, saturation, hue_degrees, alpha_post, permutation_index).  Per output pixel, in float32 (the operation
 * sequence is written out in csrc/image_prep_arith.h):
 *   position    det = a * d - b * c; u = X + 0.5 - tx, v = Y + 0.5 - ty; sx = (d * u - b * v) / det - 0.5,
 *               sy = (a * v - c * u) / det - 0.5; an image whose matrix entries, det or 1 / det are not finite, or det == 0,
 *               is outside everywhere
 *   sample      bilinear over the four neighbours of (floor(sx), floor(sy)); a neighbour outside the valid region is 0;
 *               the range is checked before any float -> int conversion
 *   colour      v = value / 255; clamp(v + delta); clamp(v * alpha_pre); saturation (multiplied, not clamped) and hue
 *               (degrees, mod 360) in HSV space, the channel order from params->is_bgr; clamp(v * alpha_post); the channel
 *               permutation of get_color_channel_permutation (an index outside 0..5 is 0); clamp(v); clamp is to [0, 1];
 *               a stage whose value is the identity (0, 1, 1 and 0, 1) is skipped, so an identity row equals null bit for bit
 *   normalise   out = (255 * v - mean[k]) / std[k] per OUTPUT channel k, folded to v * scale + bias (float64, rounded once)
 *   padding     the output extent is (ceil(output_h / tile_h) * tile_h, likewise w); padding pixels hold (0 - mean) / std
 *               with pad_before_normalize (the padder in front of the normaliser), else 0
 * out: [batch, 3, Hp, Wp] (ACCV_IP_LAYOUT_CHW) or [batch, Hp, Wp, 3] (ACCV_IP_LAYOUT_HWC) of dtype 0 f32, 1 f16, 2 bf16 (the
 * float32 result rounded once to nearest even); every element is written exactly once, nothing is read or cleared.  One
 * workgroup per (image, ACCV_IP_TILE_W x ACCV_IP_TILE_H tile of the padded output), 4 consecutive x per lane, stores of 16
 * bytes (8 for the 16-bit types) when Wp % 4 == 0 and out is aligned to the store, else per element; no workspace, no
 * atomics, no host synchronisation, bitwise reproducible.  batch == 0 launches nothing.  Returns ACCV_EINVAL (null params,
 * negative batch, an extent or tile outside [1, ACCV_IP_MAX_EXTENT], output != source extent without transforms, unknown
 * layout or dtype, mean / std not finite or std <= 0, null or misaligned pointers, more workgroups than a grid holds) before
 * touching the device, ACCV_ELAUNCH if the launch fails.  accv_prepare_images_host runs the same operation sequence serially
 * on host memory and is bit-equal; coords, when not null, receives f32 [batch, output_h, output_w, 4] rows (x0, y0, wx, wy):
 * the sample position of every output pixel, (-2, -2, 0, 0) where no neighbour can lie inside. */
#define ACCV_IP_MAX_EXTENT 16384
#define ACCV_IP_TILE_W 64
#define ACCV_IP_TILE_H 16
#define ACCV_IP_LAYOUT_CHW 0
#define ACCV_IP_LAYOUT_HWC 1
/* host memory, read during the call */
typedef struct accv_prepare_images_params {
    long long batch;
    long long source_h, source_w;           /* of the images tensor */
    long long output_h, output_w;           /* before padding */
    long long tile_h, tile_w;               /* the output is padded to multiples of these; 1: no padding */
    double mean[3], std[3];                 /* in 0..255 units, output-channel order */
    int pad_before_normalize;
    int is_bgr;
    int layout;                             /* ACCV_IP_LAYOUT_* */
    int dtype;                              /* 0 f32, 1 f16, 2 bf16 */
    int source_hw_i64;
} accv_prepare_images_params;
int accv_prepare_images(const unsigned char* images, const void* source_hw, const float* transforms, const float* photometric,
                        const accv_prepare_images_params* params, void* out, void* stream);
int accv_prepare_images_host(const unsigned char* images, const void* source_hw, const float* transforms,
                             const float* photometric, const accv_prepare_images_params* params, void* out, float* coords);

/* --------------------------------------------------------------------------------------------------------- NV12 surfaces
 * What a hardware video or JPEG decoder hands out: a pitched Y plane and an interleaved, 2 x 2 subsampled UV plane.  The
 * reference converts them in on_demand_video_decoder (convert_nv12_to_rgb, ColorConvertKernels.cu); the per-pixel
 * arithmetic is written out in csrc/nv12_arith.h: chroma sample (y / 2, x / 2) taken nearest; limited range in int32
 * fixed point (bit-equal to the reference), full range in float32 with every operator one IEEE operation (the reference's
 * fast-math build may contract them into fma; this library does not).
 *
 * y: u8, pixel (b, r, x) at byte b * y_stride_batch + r * y_stride_row + x.  uv: u8, the pair of chroma sample (b, r, i) at
 * bytes b * uv_stride_batch + r * uv_stride_row + 2 i and + 1, for r < ceil(height / 2), i < ceil(width / 2); U is the even
 * byte, or V with chroma_vu (NV21).  Strides are in bytes and not negative; nothing beyond `width` bytes of a Y row and
 * 2 * ceil(width / 2) bytes of a UV row is read.  as_bgr: the triple is written as B, G, R.
 *
 * accv_nv12_to_rgb writes out, u8 [batch, height, width, 3] contiguous, every byte once: a workgroup per (image, 64 x 16
 * tile), 4 consecutive x per lane (4 Y bytes and 4 chroma bytes in, 12 bytes out as three 4-byte stores when the address is
 * aligned, per byte otherwise); no workspace, no atomics, no host synchronisation.  batch == 0 launches nothing.  Returns
 * ACCV_EINVAL (null params, negative batch or stride, an extent outside [1, ACCV_IP_MAX_EXTENT], null pointers, more
 * workgroups than a grid holds) before touching the device, ACCV_ELAUNCH if the launch fails.  accv_nv12_to_rgb_host runs
 * the same operation sequence serially on host memory and is bit-equal. */
typedef struct accv_nv12_params {
    long long batch, height, width;
    long long y_stride_batch, y_stride_row;       /* bytes */
    long long uv_stride_batch, uv_stride_row;     /* bytes */
    int full_range;
    int as_bgr;
    int chroma_vu;
} accv_nv12_params;
int accv_nv12_to_rgb(const unsigned char* y, const unsigned char* uv, const accv_nv12_params* params, unsigned char* out,
                     void* stream);
int accv_nv12_to_rgb_host(const unsigned char* y, const unsigned char* uv, const accv_nv12_params* params, unsigned char* out);

/* accv_prepare_images reading NV12 planes instead of an RGB batch: every source tap is converted to the uint8 triple that
 * accv_nv12_to_rgb would have written, and the rest is accv_prepare_images unchanged, so the result is bit-equal to
 * accv_nv12_to_rgb followed by accv_prepare_images with is_bgr = as_bgr.  prepare: as for accv_prepare_images (source_h,
 * source_w are the planes' luma extent; its is_bgr is ignored, planes->as_bgr takes its place).  planes: the strides and the
 * format (its batch, height and width are ignored).  source_hw: the valid region inside the planes; luma outside it is never
 * read, and the chroma sample of a valid pixel always lies in the plane.  Same launch shape, checks and status codes as
 * accv_prepare_images, and ACCV_EINVAL also for a null uv pointer or a negative stride. */
typedef struct accv_prepare_images_nv12_params {
    accv_prepare_images_params prepare;
    accv_nv12_params planes;
} accv_prepare_images_nv12_params;
int accv_prepare_images_nv12(const unsigned char* y, const unsigned char* uv, const void* source_hw, const float* transforms,
                             const float* photometric, const accv_prepare_images_nv12_params* params, void* out, void* stream);
int accv_prepare_images_nv12_host(const unsigned char* y, const unsigned char* uv, const void* source_hw,
                                  const float* transforms, const float* photometric,
                                  const accv_prepare_images_nv12_params* params, void* out);

/* ------------------------------------------------------------------------------------------------ centre-point decoding
 * The prediction side of a centre-point head, the inverse of accv_center_point_targets: mmdet3d's
 * CenterPointBBoxCoder.decode (core/bbox/coders/centerpoint_bbox_coders.py: the gathers, exp, atan2, the affine map back
 * to metres, the score and post_center_range masks and the boolean index per frame) and the `circle` branch of
 * CenterHead.get_bboxes (models/dense_heads/centerpoint_head.py: circle_nms, a numba loop on the host, and the
 * post_max_size cut) for every task of the head in ONE launch, without a host round trip.
 *
 * Per task t: the peaks scores[t] [B, K] (dtype score_dtype: 0 f32, 1 f16, 2 bf16), indices[t] and classes[t] int64
 * [B, K] (what accv_heatmap_peaks writes with per_class == 0), 1 <= K <= ACCV_CD_MAX_K, in rank order; and num_maps[t]
 * (1..ACCV_CD_MAX_MAPS) maps [B, channels[t][i], H, W] contiguous of dtype map_dtype, read in place, whose channels
 * concatenate to C = 8 or 10 (the same for every task): (off_x, off_y, z, d0, d1, d2, sin, cos[, vx, vy]).
 * class_ids holds the global class ids of task 0, then of task 1, ...; task t owns class_ids[task_first[t] ..
 * task_first[t + 1]), so classes[t][b, k] is a position below task_first[t + 1] - task_first[t].
 * Per (b, t, k), in float32 (the operation sequence is written out in csrc/center_decode_arith.h, nothing contracted):
 *   legal     0 <= index < H * W and 0 <= class position < the task's class count; nothing is read for an illegal peak
 *   centre    x = ((index % W + off_x) * out_size_factor) * voxel_size[0] + pc_range[0], y likewise from index / W
 *   score     scores[b, k], or 1 / (1 + exp(-scores[b, k])) with scores_are_logits
 *   valid     legal && (no threshold || score > score_threshold) && (no range || post_center_range[0:3] <= (x, y, z) <=
 *             post_center_range[3:6]); NaN fails
 *   circle    with has_nms[t]: in rank order a valid peak is kept iff no earlier kept peak j has
 *             (x - xj)^2 + (y - yj)^2 <= nms_threshold[t] (the squared distance against the threshold as given, mmdet3d's
 *             rule); class-agnostic inside the task; a NaN distance suppresses nothing
 *   written   the first M kept peaks in rank order: boxes row (x, y, z, dims, atan2(sin, cos)[, vx, vy]), dims = exp(d)
 *             with norm_bbox, z - dims[2] * 0.5 with bottom_center (after the range test); the score; the global class id;
 *             source = k
 * Outputs, [T, B, M, ...] contiguous with 1 <= M <= K: boxes f32 [.., C - 1], out_scores f32, labels int64, source int32,
 * out_sizes int64 [T, B] (min(kept, M)).  Slots from out_sizes on are written too: +0 everywhere, source -1 (a complete
 * write).  One workgroup per (frame, task), no atomics, no workspace, no host synchronisation, bitwise reproducible.
 * B == 0 launches nothing and writes nothing.  Returns ACCV_EINVAL (null params, negative size, T outside
 * 1..ACCV_CD_MAX_TASKS, K outside 1..ACCV_CD_MAX_K, M outside 1..K, a map count outside 1..ACCV_CD_MAX_MAPS, channels that
 * do not add up to the same 8 or 10 for every task, an unknown dtype, an inconsistent class table, non-positive voxel
 * size / out_size_factor, NaN in a threshold or range, W or H < 1 or W * H >= 2^31, null or misaligned pointers) before
 * touching the device, ACCV_ELAUNCH if the launch fails.
 * accv_center_point_decode_host runs the same operation sequence serially on host memory. */
#define ACCV_CD_MAX_TASKS 8
#define ACCV_CD_MAX_MAPS 8
#define ACCV_CD_MAX_CLASSES 64
#define ACCV_CD_MAX_K 1024
/* the per-task pointers, the scalar parameters and the class table: host memory, read during the call */
typedef struct accv_center_point_decode_params {
    const void* scores[ACCV_CD_MAX_TASKS];
    const long long* indices[ACCV_CD_MAX_TASKS];
    const long long* classes[ACCV_CD_MAX_TASKS];
    const void* maps[ACCV_CD_MAX_TASKS][ACCV_CD_MAX_MAPS];
    int channels[ACCV_CD_MAX_TASKS][ACCV_CD_MAX_MAPS];
    int num_maps[ACCV_CD_MAX_TASKS];
    int has_nms[ACCV_CD_MAX_TASKS];
    double nms_threshold[ACCV_CD_MAX_TASKS];
    double pc_range[2];             /* x, y of the range's lower corner */
    double voxel_size[2];           /* x, y; > 0 */
    double out_size_factor;         /* > 0 */
    double score_threshold;
    double post_center_range[6];
    int score_dtype, map_dtype;     /* 0 f32, 1 f16, 2 bf16 */
    int num_tasks;                  /* T */
    int has_score_threshold, has_post_center_range, scores_are_logits, norm_bbox, bottom_center;
    unsigned char task_first[ACCV_CD_MAX_TASKS + 1];
    unsigned char class_ids[ACCV_CD_MAX_CLASSES];
} accv_center_point_decode_params;
int accv_center_point_decode(const accv_center_point_decode_params* params, long long B, long long K, long long H,
                             long long W, long long M, float* boxes, float* out_scores, long long* labels, int* source,
                             long long* out_sizes, void* stream);
int accv_center_point_decode_host(const accv_center_point_decode_params* params, long long B, long long K, long long H,
                                  long long W, long long M, float* boxes, float* out_scores, long long* labels, int* source,
                                  long long* out_sizes);

/* ------------------------------------------------------------------------------------- rotated BEV IoU and rotated NMS
 * The `rotate` branch of mmdet3d's CenterHead.get_bboxes (nms_bev over mmcv's nms_rotated) and the IoU underneath it
 * (mmcv's box_iou_rotated), on the device, ragged, for every task in one launch.  A BEV box is (x, y, dx, dy, yaw).  The
 * float32 operation sequence is written out in csrc/rotated_iou_arith.h: A is moved into B's frame, its corner polygon is
 * clipped (Sutherland-Hodgman) against B's four axis-aligned half-planes, the area is the shoelace sum relative to the first
 * vertex, iou = inter / (dxA * dyA + dxB * dyB - inter).  A box whose five values are not all finite, or with dx <= 0 or
 * dy <= 0, has IoU +0 with every box; boxes whose circumscribed circles are apart have IoU +0 (an exact reject).
 *
 * accv_rotated_iou_bev: a [B, Na, 5] and b [B, Nb, 5] float32 contiguous with int64 sizes [B] each (clamped to [0, Na] /
 * [0, Nb]); out [B, Na, Nb] float32, out[f, i, j] = IoU of a[f, i] against b[f, j], +0 where i or j is beyond its size;
 * every element is written exactly once.  B, Na or Nb == 0 launches nothing.
 *
 * accv_rotated_nms_bev: per task t the inputs boxes[t] [B, N, D] f32 (BEV columns 0, 1, 3, 4, 6), scores[t] [B, N] f32,
 * labels[t] [B, N] int64, source[t] [B, N] int32 and sizes[t] [B] int64: what accv_center_point_decode writes without NMS.
 * Per (b, t) only the first n = min(sizes[t][b], pre_max_size) slots exist, and the slot order is the priority order
 * (nothing is sorted).  With has_threshold[t]: walking the slots in order, a box is kept iff no earlier kept box has
 * iou > iou_threshold[t] with it (strictly: mmcv's rule); a box that is not ok is kept and suppresses nothing.  Without: every
 * slot is kept.  The first M kept rows go to output slots 0 .. in slot order, all D columns, score, label and source bit for
 * bit.  Outputs, [T, B, M, ...] contiguous with 1 <= M <= min(N, pre_max_size): boxes f32 [.., D], scores f32, labels int64,
 * source int32, out_sizes int64 [T, B] (min(kept, M)); slots from out_sizes on are written too: +0 everywhere, source -1.
 * One workgroup per (frame, task), no atomics, no workspace, no host synchronisation, bitwise reproducible.  B == 0 launches
 * nothing.  Limits: 1 <= T <= ACCV_RN_MAX_TASKS, 1 <= N <= ACCV_RN_MAX_N, ACCV_RN_MIN_D <= D <= ACCV_RN_MAX_D.
 * Both return ACCV_EINVAL (negative or oversized extent, a NaN threshold, null or misaligned pointers) before touching the
 * data, ACCV_ELAUNCH if the launch fails.  The _host entries run the same operation sequence serially on host memory. */
#define ACCV_RN_MAX_TASKS 8
#define ACCV_RN_MAX_N 1024
#define ACCV_RN_MIN_D 7
#define ACCV_RN_MAX_D 16
/* the per-task pointers and thresholds: host memory, read during the call */
typedef struct accv_rotated_nms_params {
    const float* boxes[ACCV_RN_MAX_TASKS];
    const float* scores[ACCV_RN_MAX_TASKS];
    const long long* labels[ACCV_RN_MAX_TASKS];
    const int* source[ACCV_RN_MAX_TASKS];
    const long long* sizes[ACCV_RN_MAX_TASKS];
    double iou_threshold[ACCV_RN_MAX_TASKS];
    int has_threshold[ACCV_RN_MAX_TASKS];
    int num_tasks;                  /* T */
} accv_rotated_nms_params;
int accv_rotated_iou_bev(const float* a, const long long* a_sizes, const float* b, const long long* b_sizes, long long B,
                         long long Na, long long Nb, float* out, void* stream);
int accv_rotated_iou_bev_host(const float* a, const long long* a_sizes, const float* b, const long long* b_sizes, long long B,
                              long long Na, long long Nb, float* out);
int accv_rotated_nms_bev(const accv_rotated_nms_params* params, long long B, long long N, long long D, long long pre_max_size,
                         long long M, float* boxes, float* scores, long long* labels, int* source, long long* out_sizes,
                         void* stream);
int accv_rotated_nms_bev_host(const accv_rotated_nms_params* params, long long B, long long N, long long D,
                              long long pre_max_size, long long M, float* boxes, float* scores, long long* labels, int* source,
                              long long* out_sizes);

/* ------------------------------------------------------------------------- 2D box decoding and axis-aligned NMS
 * The prediction side of a CenterNet / FCOS-style camera head, the inverse of accv_box_heatmap: mmdet's
 * CenterNetHead._decode_heatmap (models/dense_heads/centernet_head.py: transpose_and_gather_feat of the offset and size
 * maps at the top-k indices, the corner arithmetic, the rescale to the image) and the NMS behind it (batched_nms of
 * mmcv/ops/nms.py over torchvision.ops.nms: greedy, iou > threshold suppresses, classes kept apart; without its
 * coordinate-offset trick, the classes are compared) per frame in ONE launch, without a host round trip.
 *
 * accv_box_decode: the peaks scores [F, K] (dtype score_dtype: 0 f32, 1 f16, 2 bf16), indices and classes int64 [F, K] (what
 * accv_heatmap_peaks writes with per_class == 0), 1 <= K <= ACCV_BD_MAX_K, in rank order; and num_maps (1..ACCV_BD_MAX_MAPS)
 * maps [F, channels[i], Hm, Wm] contiguous of dtype map_dtype, read in place, whose channels concatenate to 4 + E,
 * 0 <= E <= ACCV_BD_MAX_EXTRAS: (off_x, off_y, h, w, extras) in map pixels, the layout of accv_box_heatmap's center_offset and
 * height_width.  The image extent is (image_h, image_w), or row f of image_hw [F, 2] int32 (int64 with image_hw_i64) as
 * (H, W) when image_hw is not null; clamped to [0, 2^24].  image_matrices: null, or f32 [F, 2, 3], the forward matrix of
 * accv_prepare_images / accv_camera_boxes.  Per (f, k), in float32 (the operation sequence is written out in
 * csrc/box_decode_arith.h, nothing contracted):
 *   legal     0 <= index < Hm * Wm and class >= 0; nothing is read from the maps for an illegal peak
 *   box       cx = index % Wm + off_x, cy = index / Wm + off_y; corners cx -+ 0.5 * w, cy -+ 0.5 * h; times ux = Wi / Wm and
 *             uy = Hi / Hm; with clip clamped to [0, Wi] / [0, Hi]
 *   score     scores[f, k], or 1 / (1 + exp(-scores[f, k])) with scores_are_logits
 *   valid     legal && (no threshold || score > score_threshold) && (no min_size || (y2 - y1 >= min_size[0] &&
 *             x2 - x1 >= min_size[1])) && the four corners are finite; NaN fails
 *   nms       with has_iou_threshold: in rank order a valid peak is kept iff no earlier kept peak (of the same class, unless
 *             class_agnostic) has iou > iou_threshold with it, strictly; iou = inter / (area_a + area_b - inter); a NaN
 *             iou suppresses nothing
 *   written   the first M kept peaks in rank order: the box, with image_matrices its two corners through the inverse of
 *             the frame's matrix (ordered per axis with order_corners; (0, 0, 0, 0) for a matrix that is singular or not
 *             finite); the score; the class; source = k; the E extra channels
 * accv_box_nms: the same NMS on boxes [F, N, 4] f32 xyxy, scores [F, N] f32, labels [F, N] int64, source [F, N] int32,
 * extras [F, N, E] f32 and sizes [F] int64: what accv_box_decode writes without NMS.  Only the first
 * n = min(sizes[f], pre_max_size) slots exist, the slot order is the priority order (nothing is sorted), a box with a
 * coordinate that is not finite is kept and suppresses nothing, without has_threshold every slot is kept; kept rows pass
 * through bit for bit.  1 <= N <= ACCV_BD_MAX_K, 1 <= M <= min(N, pre_max_size).
 * Outputs of both, [F, M, ...] contiguous: boxes f32 [.., 4], scores f32, labels int64, source int32, extras f32 [.., E]
 * (may be null with E == 0), out_sizes int64 [F] (min(kept, M)).  Slots from out_sizes on are written too: +0 everywhere,
 * source -1 (a complete write).  One workgroup per frame, no atomics, no workspace, no host synchronisation, bitwise
 * reproducible.  F == 0 launches nothing and writes nothing.  Both return ACCV_EINVAL (null params, negative or oversized
 * extent, channels that do not add up to 4..8, an unknown dtype, NaN in a threshold or min_size, null or misaligned
 * pointers) before touching the data, ACCV_ELAUNCH if the launch fails.
 * accv_box_decode_cpu and accv_box_nms_cpu run the same operation sequence serially on host memory. */
#define ACCV_BD_MAX_K 1024
#define ACCV_BD_MAX_MAPS 8
#define ACCV_BD_MAX_EXTRAS 4
/* the pointers and scalar parameters of a decode: host memory, read during the call */
typedef struct accv_box_decode_params {
    const void* scores;
    const long long* indices;
    const long long* classes;
    const void* maps[ACCV_BD_MAX_MAPS];
    int channels[ACCV_BD_MAX_MAPS];
    int num_maps;
    int image_hw_i64;
    const void* image_hw;           /* [F, 2] rows (H, W), or null: image_h, image_w for every frame */
    const float* image_matrices;    /* [F, 2, 3], or null */
    long long image_h, image_w;
    double score_threshold;
    double min_size[2];             /* (h, w) in image pixels */
    double iou_threshold;
    int score_dtype, map_dtype;     /* 0 f32, 1 f16, 2 bf16 */
    int has_score_threshold, has_min_size, has_iou_threshold;
    int scores_are_logits, clip, order_corners, class_agnostic;
} accv_box_decode_params;
/* the inputs and the threshold of an NMS: host memory, read during the call */
typedef struct accv_box_nms_params {
    const float* boxes;
    const float* scores;
    const long long* labels;
    const int* source;
    const float* extras;            /* may be null with E == 0 */
    const long long* sizes;
    double iou_threshold;
    int has_threshold, class_agnostic;
} accv_box_nms_params;
int accv_box_decode(const accv_box_decode_params* params, long long F, long long K, long long Hm, long long Wm, long long M,
                    float* boxes, float* scores, long long* labels, int* source, float* extras, long long* out_sizes,
                    void* stream);
int accv_box_decode_cpu(const accv_box_decode_params* params, long long F, long long K, long long Hm, long long Wm, long long M,
                        float* boxes, float* scores, long long* labels, int* source, float* extras, long long* out_sizes);
int accv_box_nms(const accv_box_nms_params* params, long long F, long long N, long long E, long long pre_max_size, long long M,
                 float* boxes, float* scores, long long* labels, int* source, float* extras, long long* out_sizes, void* stream);
int accv_box_nms_cpu(const accv_box_nms_params* params, long long F, long long N, long long E, long long pre_max_size,
                     long long M, float* boxes, float* scores, long long* labels, int* source, float* extras,
                     long long* out_sizes);

/* ------------------------------------------------------------------------- top-k box decoding for set-prediction heads
 * The prediction side of a DETR-style head (DETR, Deformable DETR, DINO, PETR / StreamPETR, BEVFormer, DETR3D): mmdet3d's
 * NMSFreeCoder.decode with denormalize_bbox (core/bbox/coders/nms_free_coder.py: sigmoid over all logits, topk over Q * C,
 * div and mod, gather, the element-wise decode, two masks, a boolean index per frame) and mmdet's
 * DETRHead._predict_by_feat_single, per frame in ONE launch, without a host round trip and in a defined order.
 *
 * cls_scores [B, Q, C] (dtype score_dtype: 0 f32, 1 f16, 2 bf16) and bbox_preds [B, Q, D] (dtype box_dtype), contiguous,
 * read in place.  1 <= M = max_num <= ACCV_QD_MAX_K, M <= Q * C, Q * C < 2^32 - 1.  Per frame (the operation sequence is
 * written out in csrc/query_decode_arith.h, nothing contracted):
 *   select    the M first of the Q * C raw values ranked by descending value, equal values (-0.0 == +0.0) by ascending flat
 *             index q * C + c, every NaN above +inf: torch.sort(descending, stable)[:M], the order of accv_heatmap_peaks;
 *             q = index / C, label = index % C
 *   score     the raw value, or 1 / (1 + exp(-value)) with scores_are_logits
 *   3d row    D = 8 or 10, (cx, cy, log w, log l, cz, log h, sin, cos[, vx, vy]) -> (cx, cy, cz, exp w, exp l, exp h,
 *             atan2(sin, cos)[, vx, vy]), D - 1 values; valid iff (no threshold || score > score_threshold) && (no range ||
 *             post_center_range[0:3] <= (cx, cy, cz) <= post_center_range[3:6]); with bottom_center the written z is
 *             cz - exp h * 0.5, after the range test
 *   2d row    D = 4; cxcywh: (cx -+ 0.5 * w, cy -+ 0.5 * h), else xyxy as it is; with normalized x * Wi, y * Hi; with clip
 *             clamped to [0, Wi] / [0, Hi]; valid iff (no threshold || score > score_threshold) && the four coordinates are
 *             finite; with image_matrices the written corners go through the inverse of the frame's matrix as in
 *             accv_box_decode (ordered per axis with order_corners; (0, 0, 0, 0) for a matrix that is singular or not
 *             finite).  The image extent is (image_h, image_w), or row b of image_hw [B, 2] int32 (int64 with
 *             image_hw_i64) as (H, W) when image_hw is not null; clamped to [0, 2^24]
 *   written   the valid ranks in rank order; source = q.  NaN fails every comparison
 * Outputs, [B, M, ...] contiguous: boxes f32 [.., D - 1] (3d) or [.., 4] (2d), scores f32, labels int64, source int32,
 * out_sizes int64 [B].  Slots from out_sizes on are written too: +0 everywhere, source -1 (a complete write).  One
 * workgroup per frame, no atomics on global memory, no workspace, no host synchronisation, bitwise reproducible.  B == 0
 * launches nothing and writes nothing.  Both return ACCV_EINVAL (null params, negative or oversized extent, a D other than
 * 8 / 10, an unknown dtype, NaN in a threshold or range, null or misaligned pointers) before touching the data,
 * ACCV_ELAUNCH if the launch fails.
 * accv_query_decode_3d_cpu and accv_query_decode_2d_cpu run the same operation sequence serially on host memory (the
 * selection as a stable sort on the same keys). */
#define ACCV_QD_MAX_K 1024
/* the pointers and scalar parameters of a decode: host memory, read during the call */
typedef struct accv_query_decode_3d_params {
    const void* cls_scores;
    const void* bbox_preds;
    double score_threshold;
    double post_center_range[6];    /* (x0, y0, z0, x1, y1, z1) */
    int score_dtype, box_dtype;     /* 0 f32, 1 f16, 2 bf16 */
    int has_score_threshold, has_post_center_range;
    int scores_are_logits, bottom_center;
} accv_query_decode_3d_params;
typedef struct accv_query_decode_2d_params {
    const void* cls_scores;
    const void* bbox_preds;
    const void* image_hw;           /* [B, 2] rows (H, W), or null: image_h, image_w for every frame */
    const float* image_matrices;    /* [B, 2, 3], or null */
    long long image_h, image_w;
    double score_threshold;
    int score_dtype, box_dtype;     /* 0 f32, 1 f16, 2 bf16 */
    int image_hw_i64, has_score_threshold;
    int scores_are_logits, cxcywh, normalized, clip, order_corners;
} accv_query_decode_2d_params;
int accv_query_decode_3d(const accv_query_decode_3d_params* params, long long B, long long Q, long long C, long long D, long long M,
                         float* boxes, float* scores, long long* labels, int* source, long long* out_sizes, void* stream);
int accv_query_decode_3d_cpu(const accv_query_decode_3d_params* params, long long B, long long Q, long long C, long long D,
                             long long M, float* boxes, float* scores, long long* labels, int* source, long long* out_sizes);
int accv_query_decode_2d(const accv_query_decode_2d_params* params, long long B, long long Q, long long C, long long M, float* boxes,
                         float* scores, long long* labels, int* source, long long* out_sizes, void* stream);
int accv_query_decode_2d_cpu(const accv_query_decode_2d_params* params, long long B, long long Q, long long C, long long M,
                             float* boxes, float* scores, long long* labels, int* source, long long* out_sizes);

/* --------------------------------------------------------------------------------------------- lidar depth targets
 * The depth supervision of an LSS head (BEVDepth, BEVDet4D-Depth, BEVStereo) in ONE launch: replaces the loader's
 * per-camera CPU pass (BEVDepth's map_pointcloud_to_image and depth_transform: numpy matmul, mask, a scatter into a
 * full-resolution H x W map) and the head's device pass over [B, N, H, W] (get_downsampled_gt_depth: reshape, min over
 * stride x stride blocks, bin index, one-hot).
 *
 * points [B, P, D] f32, D >= 3, contiguous: channels 0..2 are x, y, z, the rest is never read; sample_sizes [B] int32
 * (int64 with sizes_i64), clamped to [0, P], slots from it on are never read.  projection [B, C, R, 4] f32, R = 3 or 4,
 * 1 <= C <= ACCV_DT_MAX_CAMERAS, lidar to image pixels; row 3 is never read.  image_transforms [B, C, 2, 3] f32 or null: the
 * forward image matrix, folded into rows 0 and 1 exactly as accv_camera_boxes writes its projection matrices.
 * 1 <= image_h, image_w <= 2^24, downsample >= 1; the maps are h x w = ceil(image_h / downsample) x ceil(image_w / downsample),
 * w <= ACCV_DT_BAND_CELLS.  0 < depth_min < depth_max, finite.  bin_count = 0: no bins (bins may be null); else
 * 1 <= bin_count <= ACCV_DT_MAX_BINS, bin_step > 0, bin_lo and bin_step finite.  The scalars are rounded to float32 once.
 * Per (b, c) and real point, in float32 (csrc/depth_targets_arith.h, nothing contracted):
 *   p_k = ((m_k0*x + m_k1*y) + m_k2*z) + m_k3, k = 0, 1, 2;  d = p_2, u = p_0 / d, v = p_1 / d
 *   the point counts iff d >= depth_min && d < depth_max && u >= 0 && u < image_w && v >= 0 && v < image_h (NaN fails)
 *   its cell is (int(v) / downsample, int(u) / downsample)
 *   depth[b, c, cy, cx] = the smallest d of the cell, +0 where there is none
 *   bins[b, c, cy, cx]  = int(t), t = (depth - bin_lo) / bin_step, if the cell has a point, t >= 0 and int(t) < bin_count;
 *                         else -1
 * Outputs depth f32 and bins int32, [B, C, h, w] contiguous, every element written exactly once.  Output-stationary: the
 * map of a (b, c) is cut into bands of band_rows whole rows (0: chosen by the library; band_rows * w <=
 * ACCV_DT_BAND_CELLS), the grid is (bands, C, B), B <= 65535; a workgroup keeps its band in LDS, streams the frame's points
 * and takes an LDS atomic minimum on the bit pattern of d.  No atomics on global memory, no workspace, no clear, no host
 * synchronisation; the minimum does not depend on the order, so the result is bitwise reproducible and the same for every
 * band_rows.  B == 0 launches nothing and writes nothing; P == 0 writes +0 and -1.  ACCV_EINVAL (null params, a size or
 * scalar outside the ranges above, null or misaligned pointers) before touching the data, ACCV_ELAUNCH if the launch fails.
 * accv_depth_targets_cpu runs the same operation sequence serially on host memory. */
#define ACCV_DT_MAX_CAMERAS 16
#define ACCV_DT_BAND_CELLS 8192
#define ACCV_DT_MAX_BINS 32768
/* the inputs and scalar parameters of a call: host memory, read during the call */
typedef struct accv_depth_targets_params {
    const float* points;
    const void* sample_sizes;
    const float* projection;
    const float* image_transforms;  /* or null */
    long long image_h, image_w;
    double depth_min, depth_max;
    double bin_lo, bin_step;
    int downsample, bin_count;      /* bin_count 0: no bins */
    int sizes_i64, band_rows;       /* band_rows 0: automatic */
} accv_depth_targets_params;
int accv_depth_targets(const accv_depth_targets_params* params, long long B, long long P, long long D, long long C, long long R,
                       float* depth, int* bins, void* stream);
int accv_depth_targets_cpu(const accv_depth_targets_params* params, long long B, long long P, long long D, long long C,
                           long long R, float* depth, int* bins);

/* ------------------------------------------------------------------------------------------------- hard voxelization
 * The pass from the lidar points of a batch of frames to the voxels or pillars the network reads: replaces mmcv's
 * Voxelization (hard_voxelize_forward; spconv's points_to_voxel is the same rule), which mmdet3d calls once per frame in a
 * Python loop (Base3DDetector.voxelize) and whose GPU kernel hands out voxel numbers with an atomic counter.  The result
 * here is the one of the SEQUENTIAL loop (hard_voxelize_forward_cpu), bit for bit, on the device and on the host.
 *
 * points [B, P, D] f32, ACCV_VX_MIN_D <= D <= ACCV_VX_MAX_D, contiguous: channels 0..2 are x, y, z, the rest passes through;
 * sample_sizes [B] int32 (int64 with sizes_i64), clamped to [0, P], slots from it on are never read.  augmentation
 * [B, 7] f32 or null: the rows (θ, c, s, k, tx, ty, tz) of accv_bev_augment; x, y, z go through its augment_center before
 * the voxel test and are stored augmented.  voxel_size (vx, vy, vz) > 0, range_min < range_max, all finite, rounded to
 * float32 once; the grid is g_k = rint((hi_k - lo_k) / v_k) in float32, each g_k >= 1, g_x * g_y * g_z < 2^31.
 * 1 <= max_points = T <= ACCV_VX_MAX_POINTS, 1 <= max_voxels = V <= ACCV_VX_MAX_VOXELS, B <= 65535, P < 2^31 - 1.
 * Per frame, points in slot order, float32, nothing contracted (csrc/voxelize_arith.h):
 *   t_k = floor((p_k - lo_k) / v_k); in range iff t_k >= 0 && t_k < (float)g_k for k = x, y, z (float compares: NaN, +inf and
 *   -inf fail; mmcv casts first);  c_k = (int)t_k,  key = (c_z * g_y + c_y) * g_x + c_x
 *   a key without a voxel: with V voxels open the point is skipped AND THE LOOP GOES ON (mmcv's `continue`, not the older
 *   `break`); else the voxel takes the next number and coors = (c_z, c_y, c_x)
 *   a voxel with fewer than T points stores the point's D channels in its next row (x, y, z augmented, the rest bit for bit)
 * Outputs, every element written exactly once: voxels f32 [B, V, T, D] (+0 rows from num_points on and in voxels from
 * voxel_counts on), coors int32 [B, V, 3] (-1 from voxel_counts on), num_points int32 [B, V] (0 from voxel_counts on),
 * voxel_counts int32 [B], point_voxel int32 [B, P] or null (the voxel number of each point, also of a point beyond T; -1 out
 * of range, beyond sample_sizes or refused by V).
 * Device: one hipMemsetAsync and five launches on `stream` (insert and rank: a lane per point; count and number: a
 * workgroup per chunk of 4096 points of a frame, further workgroups of count fill the index lists; gather: a lane per 16 or
 * 4 bytes of voxels; three launches when P == 0), no host synchronisation, capturable.  No atomic decides an order: a per-frame hash table (table_slots slots, 0 = the power of
 * two that is at least 2 * P; else a power of two above P, at most 2^31) keeps the lowest point index per key, a prefix sum
 * over the points numbers the voxels, and a bounded atomicMin cascade sorts each voxel's first T indices.  workspace:
 * accv_voxelize_workspace_bytes(B, P, V, T, table_slots) bytes of device memory, 16-byte aligned (0 for sizes the call
 * refuses).  B == 0 launches nothing; P == 0 still writes all padding.  ACCV_EINVAL (null params, a size or scalar outside
 * the ranges above, null or misaligned pointers) or ACCV_EWORKSPACE before touching the data, ACCV_ELAUNCH if a launch
 * fails.  accv_voxelize_cpu runs the sequential loop over the same arithmetic on host memory and needs no workspace. */
#define ACCV_VX_MIN_D 3
#define ACCV_VX_MAX_D 16
#define ACCV_VX_MAX_POINTS 128
#define ACCV_VX_MAX_VOXELS 1048576
/* the inputs and scalar parameters of a call: host memory, read during the call */
typedef struct accv_voxelize_params {
    const float* points;
    const void* sample_sizes;
    const float* augmentation;      /* or null */
    double voxel_size[3];           /* x, y, z */
    double range_min[3], range_max[3];
    long long table_slots;          /* 0: automatic */
    int max_points, max_voxels;
    int sizes_i64;
} accv_voxelize_params;
size_t accv_voxelize_workspace_bytes(long long B, long long P, long long V, long long T, long long table_slots);
int accv_voxelize(const accv_voxelize_params* params, long long B, long long P, long long D, float* voxels, int* coors,
                  int* num_points, int* voxel_counts, int* point_voxel, void* workspace, size_t workspace_bytes, void* stream);
int accv_voxelize_cpu(const accv_voxelize_params* params, long long B, long long P, long long D, float* voxels, int* coors,
                      int* num_points, int* voxel_counts, int* point_voxel);

/* ------------------------------------------------------------------------------- pillar decoration and the voxel mean
 * From the voxels of accv_voxelize to the rows a pillar feature net's first linear layer reads: mmdet3d's non-legacy
 * PillarFeatureNet.forward up to that layer (accv_pillar_features) and HardSimpleVFE (accv_voxel_mean), one launch each.
 *
 * voxels [M, T, D] f32 contiguous, ACCV_VX_MIN_D <= D <= ACCV_VX_MAX_D, 1 <= T <= ACCV_VX_MAX_POINTS; num_points [M] int32,
 * clamped to [0, T]; coors [M, coor_width] int32 with coor_width 3 (z, y, x) or 4 (b, z, y, x): the last three columns are
 * read.  voxel_size > 0 and range_min finite, rounded to float32 once.  Per voxel, float32, nothing contracted
 * (csrc/pillar_features_arith.h):
 *   n = clamp(num_points, 0, T);  s_k = ((p_0k + p_1k) + p_2k) + ... over the rows j < n in row order, k = x, y, z
 *   mean_k = s_k / float(n);  centre_k = float(c_k) * v_k + (v_k * 0.5f + lo_k), c = (x, y, z) from the last coors columns
 *   a row j < n: [the D input channels bit for bit | p_jk - mean_k (ACCV_PF_CLUSTER) | p_jk - centre_k (ACCV_PF_CENTER) |
 *   sqrt((x * x + y * y) + z * z) (ACCV_PF_DISTANCE)];  a row j >= n: +0.0 in every channel, whatever the input holds there
 * out f32 [M, T, F], F = D + 3 per CLUSTER and CENTER + 1 for DISTANCE, every element written exactly once.
 * accv_voxel_mean: out f32 [M, num_features], the same s_k / float(n) over the first 1 <= num_features <= D channels, +0.0
 * where n == 0.  Device: one launch on `stream`; a workgroup stages as many consecutive voxels as fit its LDS budget (16-byte
 * loads where the voxels and the workgroup's range are 16-byte aligned), sums from LDS, a lane per (voxel, channel), and all
 * lanes write the rows; no workspace, no atomics, nothing read but the three inputs.  M == 0 launches nothing.  ACCV_EINVAL
 * (null params, sizes or scalars outside the ranges above, null or misaligned pointers) before touching the data,
 * ACCV_ELAUNCH if the launch fails.  The _cpu entries evaluate the same arithmetic on host memory. */
#define ACCV_PF_CLUSTER 1u
#define ACCV_PF_CENTER 2u
#define ACCV_PF_DISTANCE 4u
typedef struct accv_pillar_features_params {
    const float* voxels;
    const int* num_points;
    const int* coors;
    double voxel_size[3];           /* x, y, z */
    double range_min[3];
    int coor_width;                 /* 3 or 4 */
    unsigned flags;                 /* ACCV_PF_* */
} accv_pillar_features_params;
int accv_pillar_features(const accv_pillar_features_params* params, long long M, long long T, long long D, float* out, void* stream);
int accv_pillar_features_cpu(const accv_pillar_features_params* params, long long M, long long T, long long D, float* out);
int accv_voxel_mean(const float* voxels, const int* num_points, long long M, long long T, long long D, long long num_features,
                    float* out, void* stream);
int accv_voxel_mean_cpu(const float* voxels, const int* num_points, long long M, long long T, long long D, long long num_features,
                        float* out);

/* ------------------------------------------------------------------------------------------------------- BEV scatter
 * From per-pillar features to the dense map a 2D backbone convolves: mmdet3d's PointPillarsScatter for the whole batch, the
 * canvas written once with its zeros, and the backward of that.
 *
 * features [rows, C] of elem_size 4 (f32) or 2 (f16 / bf16: the copy moves bits), contiguous, 1 <= C <= ACCV_BS_MAX_C;
 * coors int32 [rows, coor_width]: coor_width 4 is (b, z, y, x); coor_width 3 is (z, y, x) with the frame implicit, b = r / V
 * (the padded [B, V, ...] form, rows == B * V).  Row r is placed iff 0 <= b < B, 0 <= y < ny, 0 <= x < nx; z is ignored.
 * B * ny * nx < 2^31, rows < 2^31.
 *   index [B, ny, nx] int32: the highest placed r of the cell, or -1
 *   canvas [B, C, ny, nx]: features[index[b, y, x], c], or +0 where the index is -1; every element written exactly once
 *   backward: grad_features[r, c] = grad_canvas[b, c, y, x] if index[cell(r)] == r, else +0; every element written once
 * Device, forward: one hipMemsetAsync (index = 0xFF bytes) and two launches on `stream`: mark (a lane per row, atomicMax on
 * index) and write (a workgroup per frame, map row, 64 cells along x and 64 channels: the occupied cells' feature rows through
 * LDS, 16-byte loads and stores where features, canvas, C * elem_size and nx * elem_size are 16-byte aligned, element by
 * element otherwise; a tile without rows stores zeros only).  No atomic on the canvas and no read of it.  Backward: one
 * launch, no atomics; reads coors, index and grad_canvas.  B == 0 launches nothing; rows == 0 still writes canvas and
 * index.  ACCV_EINVAL (sizes outside the ranges above, null or misaligned pointers) before touching the data, ACCV_ELAUNCH
 * if a launch fails.  The _cpu entries run the sequential loop on host memory. */
#define ACCV_BS_MAX_C 1024
int accv_bev_scatter(const void* features, const int* coors, long long rows, long long V, long long B, long long C, long long ny,
                     long long nx, int coor_width, int elem_size, void* canvas, int* index, void* stream);
int accv_bev_scatter_cpu(const void* features, const int* coors, long long rows, long long V, long long B, long long C, long long ny,
                         long long nx, int coor_width, int elem_size, void* canvas, int* index);
int accv_bev_scatter_bwd(const void* grad_canvas, const int* coors, const int* index, long long rows, long long V, long long B,
                         long long C, long long ny, long long nx, int coor_width, int elem_size, void* grad_features, void* stream);
int accv_bev_scatter_bwd_cpu(const void* grad_canvas, const int* coors, const int* index, long long rows, long long V, long long B,
                             long long C, long long ny, long long nx, int coor_width, int elem_size, void* grad_features);

/* ------------------------------------------------------------------------------------------------ batched assignment
 * Replaces the per-frame scipy.optimize.linear_sum_assignment loop of the Hungarian matcher
 * (packages/batching_helpers/example/matcher.py:52-74: cost.to_device(cpu), split, scipy per frame, combine_data, copy
 * back).  Per frame b the minimum-cost (ACCV_LSA_MAXIMIZE: maximum-cost) complete matching of the smaller side of the
 * R_b x C_b block cost[b, :R_b, :C_b], with scipy's semantics: +inf (-inf under maximize) forbids a pair, NaN and -inf
 * (+inf under maximize) are invalid entries.  Exact: shortest augmenting paths with f64 duals; argmin ties go to an
 * unassigned column, then the lowest index, so results are bitwise reproducible and equal to the host solver's.
 * cost: dtype 0 f32, 1 f16, 2 bf16, 3 f64, element (b, r, c) at cost[b * stride_b + r * stride_r + c * stride_c]
 * (strides in elements; any view).  row_counts / col_counts: device int64 [B] (R_b, C_b), NULL = R / C for every frame,
 * values clamped to [0, R] / [0, C].  Limits: max(R, C) <= 4096 and min(R, C) <= 1024 of the padded shape.
 * Outputs, W = min(R, C): row_ind / col_ind int64 [B, W] (the pairs with row_ind ascending, zero from sizes[b] on),
 * sizes int64 [B] (min(R_b, C_b), 0 for a failed frame), status int32 [B] (0 ok, 1 infeasible, 2 invalid entry).
 * One workgroup per frame; no host synchronisation.  workspace: accv_linear_assignment_workspace_bytes(B, R, C, dtype)
 * bytes of device memory, 16-byte aligned (0 for sizes the call refuses).  Returns ACCV_EINVAL (negative or oversized
 * extent, unknown dtype or flag, null pointers) or ACCV_EWORKSPACE before touching the device, ACCV_ELAUNCH if the
 * launch fails; B == 0 launches nothing. */
#define ACCV_LSA_MAXIMIZE 1u
#define ACCV_LSA_THREADS_64 2u    /* hint: one wave per frame instead of 256 lanes (same results) */
#define ACCV_LSA_THREADS_1024 4u  /* hint: 1024 lanes per frame (same results) */
size_t accv_linear_assignment_workspace_bytes(long long B, long long R, long long C, int dtype);
int accv_linear_assignment(const void* cost, int dtype, long long B, long long R, long long C, long long stride_b,
                           long long stride_r, long long stride_c, const long long* row_counts,
                           const long long* col_counts, unsigned flags, long long* row_ind, long long* col_ind,
                           long long* sizes, int* status, void* workspace, size_t workspace_bytes, void* stream);
/* The same solver on the host (same algorithm, tie rule and f64 operation sequence: equal results bit for bit); every
 * pointer is host memory.  Blocks the calling thread. */
int accv_linear_assignment_host(const void* cost, int dtype, long long B, long long R, long long C, long long stride_b,
                                long long stride_r, long long stride_c, const long long* row_counts,
                                const long long* col_counts, unsigned flags, long long* row_ind, long long* col_ind,
                                long long* sizes, int* status);

/* ------------------------------------------------------------------------------------------------ matching costs
 * The [B, Q, G] cost matrices of Hungarian matching in one launch (what accv_linear_assignment reads): replaces the
 * broadcast chains and the per-object one-hot loop of packages/batching_helpers/example/matcher.py:22-31, 78-132.
 * out[b, q, g] (contiguous, f32, f64 for dtype 3) is, for g < G_b = clamp(counts[b], 0, G) (counts: device int64 [B],
 * NULL = G for every frame):
 *     class_weight * cls + l1_weight * l1 + iou_weight * iou + giou_weight * giou     (summed in this order)
 * and params->filler for G_b <= g < G.  A term whose weight is 0 is not evaluated and its pointers may be NULL.
 *   cls (kind 0) 1 - p[q, l_g]; (kind 1) -p[q, l_g]; (kind 2) mmdet FocalLossCost with s = sigmoid(x[q, l_g]) and
 *       1 - s from exp(-|x|):  (-log(s + eps)) * alpha * (1 - s)^gamma - (-log(1 - s + eps)) * (1 - alpha) * s^gamma;
 *       a label outside [0, C) gives NaN
 *   l1   sum over d < D of |bp_d - bg_d|
 *   iou  1 - inter / max(union, iou_eps), intersection sides clamped at 0, areas not clamped
 *   giou -GIoU with union and enclosing area floored at iou_eps (mmdet bbox_overlaps, mode "giou")
 * IoU and GIoU need D == 4 and read xyxy boxes, or cxcywh boxes with ACCV_MC_CXCYWH (converted first); l1 reads the raw
 * coordinates.  NaN in an evaluated input gives NaN for the pair; infinities follow the float64 formula.
 * scores [B, Q, C] (element (b, q, c) at b * scores_stride_b + q * scores_stride_q + c), pred_boxes [B, Q, D] (the
 * same with boxes_stride_b / boxes_stride_q): dtype 0 f32, 1 f16, 2 bf16, 3 f64 (the codes of accv_linear_assignment),
 * strides in elements; gt_labels [B, G] int32 (int64 with ACCV_MC_LABELS_I64) and gt_boxes [B, G, D] of the same dtype,
 * contiguous.  f16 / bf16 are widened exactly to f32 and evaluated in f32; f64 in f64.  D <= 16.  Returns ACCV_EINVAL
 * (null params, negative size, unknown dtype, kind or flag, D > 16, IoU / GIoU with D != 4, a null pointer of an
 * evaluated term or of out) before touching the device, ACCV_ELAUNCH if the launch fails; B * Q * G == 0 launches
 * nothing.  No host synchronisation. */
#define ACCV_MC_ONE_MINUS_PROB 0
#define ACCV_MC_NEG_PROB 1
#define ACCV_MC_FOCAL 2
#define ACCV_MC_LABELS_I64 1u
#define ACCV_MC_CXCYWH 2u
/* the float parameters, host memory, read during the call (passed by pointer so the entry takes integers only) */
typedef struct accv_matching_cost_params {
    double class_weight, l1_weight, iou_weight, giou_weight;
    double focal_alpha, focal_gamma, focal_eps, iou_eps;
    double filler;
} accv_matching_cost_params;
int accv_matching_cost(const void* scores, const void* pred_boxes, const void* gt_labels, const void* gt_boxes,
                       const long long* counts, int dtype, int kind, unsigned flags, long long B, long long Q,
                       long long C, long long G, long long D, long long scores_stride_b, long long scores_stride_q,
                       long long boxes_stride_b, long long boxes_stride_q, const accv_matching_cost_params* params,
                       void* out, void* stream);
/* The same on the host (same operation sequence: equal bits for every term but the focal one); every pointer is host
 * memory.  Blocks the calling thread. */
int accv_matching_cost_host(const void* scores, const void* pred_boxes, const void* gt_labels, const void* gt_boxes,
                            const long long* counts, int dtype, int kind, unsigned flags, long long B, long long Q,
                            long long C, long long G, long long D, long long scores_stride_b, long long scores_stride_q,
                            long long boxes_stride_b, long long boxes_stride_q, const accv_matching_cost_params* params,
                            void* out);

/* ------------------------------------------------------------------------------------------------ matched focal loss
 * The sigmoid focal classification loss of a set-prediction head over ALL queries against the labels of the matched
 * ground truth (torchvision sigmoid_focal_loss / mmdet py_sigmoid_focal_loss on one-hot targets), without the [B, Q, C]
 * one-hot target and the dozen element-wise launches of the torch composition:
 *     out[b] = sum over q, c of  w[b, q] * l(x[b, q, c], c == label_b(q)) / denom
 *     l(x, positive) = alpha (1 - s)^gamma softplus(-x),  l(x, negative) = (1 - alpha) s^gamma softplus(x),  s = sigmoid(x)
 * alpha < 0 switches the alpha blend off; gamma >= 0 (2 runs as a multiplication, other values through pow).
 * label_b(q): the pairs of frame b are the slots j < n_b = clamp(counts[b], 0, K) (counts: int64 [B]) of pred_ind /
 * gt_ind [B, K] (int32, int64 with ACCV_MF_IDX_I64).  A pair names its query when 0 <= pred_ind < Q and 0 <= gt_ind < G;
 * other pairs are skipped (no wrapping).  The LOWEST slot that names q decides: label_b(q) = gt_labels[b, gt_ind[b, j]]
 * ([B, G] int32, int64 with ACCV_MF_LABELS_I64) when that lies in [0, C); otherwise, and for a query no pair names, every
 * class of q is a negative.  Slots at or past n_b are never read.
 * logits [B, Q, C] of dtype 0 f32, 1 f16, 2 bf16, 3 f64 (the codes of accv_matching_cost): element (b, q, c) at
 * b * stride_b + q * stride_q + c, strides in elements, stride_q >= C.  query_weights: NULL or contiguous [B, Q] of the
 * logits dtype.  f16 / bf16 are widened exactly and evaluated in f32, f64 in f64; sums are accumulated in f64.
 * denom: max(sum_b n_b, 1) (ACCV_FL_AVG_NUM_POS), params->avg_factor (ACCV_FL_AVG_VALUE) or *params->avg_factor_dev
 * (ACCV_FL_AVG_DEVICE, an f32 scalar in device memory; host memory for the host entry points).
 * out [B] f32 (f64 for dtype 3); out_denom one f64 scalar that the backward reads.  workspace:
 * accv_matched_focal_loss_workspace_bytes(B, Q, C) bytes of device memory, 16-byte aligned.  Two launches, no atomics
 * on global memory, no host synchronisation, bitwise reproducible.  Returns ACCV_EINVAL (null params, negative size,
 * unknown dtype / flag / avg mode, gamma < 0 or NaN, C or K above 2^31 - 1, stride_q < C, null or misaligned pointers) or
 * ACCV_EWORKSPACE before touching the device, ACCV_ELAUNCH if a launch fails.  B * Q * C == 0 launches nothing and
 * writes nothing. */
#define ACCV_MF_IDX_I64 1u
#define ACCV_MF_LABELS_I64 2u
/* the scalar parameters, host memory, read during the call (by pointer so the entries take integers only) */
typedef struct accv_matched_focal_params {
    double alpha, gamma;
    double avg_factor;           /* the denominator of ACCV_FL_AVG_VALUE */
    int avg_mode;                /* ACCV_FL_AVG_NUM_POS, ACCV_FL_AVG_VALUE or ACCV_FL_AVG_DEVICE; the backward ignores it */
    const float* avg_factor_dev; /* the f32 scalar of ACCV_FL_AVG_DEVICE */
} accv_matched_focal_params;
size_t accv_matched_focal_loss_workspace_bytes(long long B, long long Q, long long C);
int accv_matched_focal_loss(const void* logits, const void* gt_labels, const void* pred_ind, const void* gt_ind,
                            const long long* counts, const void* query_weights_or_null, int dtype, unsigned flags,
                            long long B, long long Q, long long C, long long G, long long K, long long stride_b,
                            long long stride_q, const accv_matched_focal_params* params, void* out, double* out_denom,
                            void* workspace, size_t workspace_bytes, void* stream);
/* Its backward: grad_logits (contiguous [B, Q, C], the logits dtype, round to nearest even) is written completely, every
 * element exactly once: (w[b, q] * dl/dx) * (grad_out[b] / *denom), the scale formed in f64 and rounded to the
 * arithmetic type.  grad_out [B] has the dtype of out, denom is out_denom of the forward.  One launch; needs no
 * initialised gradient, uses no atomics. */
int accv_matched_focal_loss_bwd(const void* logits, const void* gt_labels, const void* pred_ind, const void* gt_ind,
                                const long long* counts, const void* query_weights_or_null, const void* grad_out,
                                const double* denom, int dtype, unsigned flags, long long B, long long Q, long long C,
                                long long G, long long K, long long stride_b, long long stride_q,
                                const accv_matched_focal_params* params, void* grad_logits, void* stream);
/* The same on the host (same operation sequence per element; a frame's sum is accumulated in element order); every
 * pointer is host memory.  Block the calling thread. */
int accv_matched_focal_loss_host(const void* logits, const void* gt_labels, const void* pred_ind, const void* gt_ind,
                                 const long long* counts, const void* query_weights_or_null, int dtype, unsigned flags,
                                 long long B, long long Q, long long C, long long G, long long K, long long stride_b,
                                 long long stride_q, const accv_matched_focal_params* params, void* out, double* out_denom);
int accv_matched_focal_loss_bwd_host(const void* logits, const void* gt_labels, const void* pred_ind, const void* gt_ind,
                                     const long long* counts, const void* query_weights_or_null, const void* grad_out,
                                     const double* denom, int dtype, unsigned flags, long long B, long long Q, long long C,
                                     long long G, long long K, long long stride_b, long long stride_q,
                                     const accv_matched_focal_params* params, void* grad_logits);

/* -------------------------------------------------------------------------------------------------- matched box loss
 * The box regression loss of a set-prediction head over the matched pairs, both terms in one pass:
 *     out[0][b] = sum over the pairs (q, g) of frame b of  w[b, q] * sum_d cw[d] |p[b, q, d] - gt[b, g, d]| / denom
 *     out[1][b] = sum over the pairs of  w[b, q] * (1 - giou(p, gt))  (ACCV_MB_GIOU),  (1 - iou) (ACCV_MB_IOU),  0 (ACCV_MB_IOU_NONE)
 * IoU / GIoU as in accv_matching_cost (mmdet bbox_overlaps, union and enclosure floored at iou_eps, maxima and minima
 * keep NaN), boxes xyxy or, with ACCV_MB_CXCYWH, cxcywh; an IoU kind needs D == 4, the L1 term takes 1 <= D <= 16.
 * Pairs: the rule of accv_matched_focal_loss.  The slots j < n_b = clamp(counts[b], 0, K) (counts: int64 [B]) of pred_ind /
 * gt_ind [B, K] (int32, int64 with ACCV_MB_IDX_I64) name query pred_ind[b, j] when 0 <= pred_ind < Q and 0 <= gt_ind < G;
 * the LOWEST slot that names a query is its pair, other slots are skipped, slots at or past n_b are never read.
 * pred_boxes [B, Q, D] of dtype 0 f32, 1 f16, 2 bf16, 3 f64: element (b, q, d) at b * stride_b + q * stride_q + d, strides
 * in elements, stride_q >= D.  gt_boxes: contiguous [B, G, D] of the same dtype.  f16 / bf16 are widened exactly and
 * evaluated in f32, f64 in f64; sums are accumulated in f64.  denom as for accv_matched_focal_loss.
 * out: [2, B] f32 (f64 for dtype 3), row 0 the L1 sums, row 1 the IoU sums; out_denom one f64 scalar that the backward
 * reads.  workspace: accv_matched_box_loss_workspace_bytes(B, Q, D) bytes of device memory, 16-byte aligned.  Two
 * launches, no atomics on global memory, no host synchronisation, bitwise reproducible.  Returns ACCV_EINVAL (null params,
 * negative size, unknown dtype / flag / IoU kind / avg mode, D outside [1, 16], an IoU kind with D != 4, K above 2^31 - 1,
 * stride_q < D, null or misaligned pointers) or ACCV_EWORKSPACE before touching the device, ACCV_ELAUNCH if a launch
 * fails.  B * Q == 0 launches nothing and writes nothing. */
#define ACCV_MB_IDX_I64 1u
#define ACCV_MB_CXCYWH 2u
#define ACCV_MB_IOU_NONE 0
#define ACCV_MB_IOU 1
#define ACCV_MB_GIOU 2
/* the scalar parameters and optional operands, host memory, read during the call */
typedef struct accv_matched_box_params {
    double iou_eps;
    double avg_factor;            /* the denominator of ACCV_FL_AVG_VALUE */
    double code_weights[16];      /* cw[d] for d < D, rounded to the arithmetic type; read when code_weights_dev is NULL */
    int avg_mode;                 /* ACCV_FL_AVG_NUM_POS, ACCV_FL_AVG_VALUE or ACCV_FL_AVG_DEVICE; the backward ignores it */
    int iou_kind;                 /* ACCV_MB_IOU_NONE, ACCV_MB_IOU or ACCV_MB_GIOU */
    const float* avg_factor_dev;  /* the f32 scalar of ACCV_FL_AVG_DEVICE */
    const void* code_weights_dev; /* NULL or [D] of the boxes' dtype in the boxes' memory */
    const void* query_weights;    /* NULL or contiguous [B, Q] of the boxes' dtype */
} accv_matched_box_params;
size_t accv_matched_box_loss_workspace_bytes(long long B, long long Q, long long D);
int accv_matched_box_loss(const void* pred_boxes, const void* gt_boxes, const void* pred_ind, const void* gt_ind,
                          const long long* counts, int dtype, unsigned flags, long long B, long long Q, long long D, long long G,
                          long long K, long long stride_b, long long stride_q, const accv_matched_box_params* params, void* out,
                          double* out_denom, void* workspace, size_t workspace_bytes, void* stream);
/* Its backward: grad_boxes (contiguous [B, Q, D], the boxes' dtype, round to nearest even) is written completely, every
 * element exactly once: (s1 * dL1 + s2 * dIoU) * w[b, q] with s1 = grad_l1[b] / *denom and s2 = grad_iou[b] / *denom
 * formed in f64 and rounded to the arithmetic type; +0 for a query without a pair.  grad_l1 and grad_iou ([B] each, the
 * dtype of out) are the gradients of the two rows of out; either may be NULL and then counts as zeros.  denom is
 * out_denom of the forward.  The derivative follows float64 autograd over the definition: an exact tie of a
 * maximum / minimum splits evenly, a floor that fires passes nothing, |0| has derivative 0.  One launch; needs no
 * initialised gradient, uses no atomics. */
int accv_matched_box_loss_bwd(const void* pred_boxes, const void* gt_boxes, const void* pred_ind, const void* gt_ind,
                              const long long* counts, const void* grad_l1, const void* grad_iou, const double* denom, int dtype,
                              unsigned flags, long long B, long long Q, long long D, long long G, long long K, long long stride_b,
                              long long stride_q, const accv_matched_box_params* params, void* grad_boxes, void* stream);
/* The same on the host (same operation sequence per pair; a frame's sums are accumulated in query order); every pointer
 * is host memory.  Block the calling thread. */
int accv_matched_box_loss_host(const void* pred_boxes, const void* gt_boxes, const void* pred_ind, const void* gt_ind,
                               const long long* counts, int dtype, unsigned flags, long long B, long long Q, long long D,
                               long long G, long long K, long long stride_b, long long stride_q,
                               const accv_matched_box_params* params, void* out, double* out_denom);
int accv_matched_box_loss_bwd_host(const void* pred_boxes, const void* gt_boxes, const void* pred_ind, const void* gt_ind,
                                   const long long* counts, const void* grad_l1, const void* grad_iou, const double* denom,
                                   int dtype, unsigned flags, long long B, long long Q, long long D, long long G, long long K,
                                   long long stride_b, long long stride_q, const accv_matched_box_params* params,
                                   void* grad_boxes);

/* --------------------------------------------------------------- polyline matching cost and matched polyline loss
 * Set prediction over polylines (MapTR-style vectorised map heads, lane-DETR heads).  A line is P points of D coordinates
 * (2 <= P <= 128, D 2 or 3); a ground-truth line equals all of its equivalent orders t^v:
 *     open line     t^0[p] = t[p];  with ACCV_PM_REVERSIBLE also t^1[p] = t[P - 1 - p]
 *     closed line   t^s[p] = t[(s + p) mod P], s < P;  with ACCV_PM_REVERSIBLE also t^(P + s)[p] = t[(s - p) mod P]
 * gt_closed (params; NULL = every line is open) marks the closed lines: contiguous [B, G], non-zero = closed, one byte per
 * element, or four / eight with ACCV_PM_CLOSED_I32 / ACCV_PM_CLOSED_I64.  v*(x, t) is the LOWEST v that minimises
 * sum_{p, d} |x[p, d] - t^v[p, d]| in the arithmetic type (f32 for dtype 0 f32, 1 f16, 2 bf16, which are widened exactly;
 * f64 for dtype 3); the sum runs over p, d in order in partial sums of 8 points.  No order is ever written to memory.
 * pred_lines [B, Q, P, D]: element (b, q, p, d) at b * pred_stride_b + q * pred_stride_q + p * D + d (params; elements,
 * pred_stride_q >= P * D); gt_lines: contiguous [B, G, P, D] of the same dtype.
 *
 * accv_polyline_matching_cost: out[b, q, g] (contiguous [B, Q, G], f32, f64 for dtype 3) is, for g < G_b =
 * clamp(counts[b], 0, G) (counts: int64 [B], NULL = G for every frame),
 *     class_weight * cls(q, l_g) + pts_weight * min_v sum_{p, d} |x_q - t_g^v|        (summed in this order)
 * and params->filler for G_b <= g < G.  cls is the class term of accv_matching_cost (params->class_kind one of
 * ACCV_MC_ONE_MINUS_PROB / _NEG_PROB / _FOCAL; scores [B, Q, C] with scores_stride_b / scores_stride_q, gt_labels [B, G]
 * int32, int64 with ACCV_PM_LABELS_I64).  A term whose weight is 0 is not evaluated and its pointers may be NULL.  NaN
 * in a coordinate of a pair gives NaN for that pair.  One launch, no host synchronisation; B * Q * G == 0 launches nothing.
 *
 * accv_matched_polyline_loss: over the pairs of accv_matched_box_loss (the same rule: slots j < clamp(counts[b], 0, K) of
 * pred_ind / gt_ind [B, K], int32 or int64 with ACCV_PM_IDX_I64, the lowest slot that names a query with both indices in
 * range is its pair), with t* = t_g^(v*):
 *     out[0][b] = sum over the pairs of  sum_{p, d} |x[p, d] - t*[p, d]| / denom
 *     out[1][b] = sum over the pairs of  sum_s (1 - <a_s, b_s> / sqrt((|a_s|^2 + dir_eps) (|b_s|^2 + dir_eps))) / denom
 * a_s = x[s+1] - x[s], b_s = t*[s+1] - t*[s]; s = 0 .. P-2 for an open line, 0 .. P-1 with s + 1 mod P for a closed one;
 * zeros, nothing evaluated, when params->dir_loss is 0.  denom as for accv_matched_focal_loss.  out [2, B] f32 (f64 for
 * dtype 3), out_denom one f64 scalar for the backward, workspace accv_matched_polyline_loss_workspace_bytes(B, Q) bytes
 * of device memory, 16-byte aligned.  Sums are accumulated in f64 in a fixed order: two launches, no atomics on global
 * memory, no host synchronisation, bitwise reproducible.  B * Q == 0 launches nothing and writes nothing.
 * accv_matched_polyline_loss_bwd: grad_lines (contiguous [B, Q, P, D], the lines' dtype) is written completely, every
 * element exactly once, +0 for a query without a pair: s1 * sgn(x - t*) + s2 * d dir / d x with s1 = grad_pts[b] / *denom,
 * s2 = grad_dir[b] / *denom formed in f64 and rounded to the arithmetic type (either may be NULL: zeros).  v* is a constant
 * of the derivative and is searched again; sgn(0) = 0.  One launch, no atomics, no zero fill.
 * All return ACCV_EINVAL (null params, negative size, unknown dtype / flag / class kind / avg mode, P outside [2, 128],
 * D not 2 or 3, pred_stride_q < P * D, K above 2^31 - 1, null or misaligned pointers) or ACCV_EWORKSPACE before touching the
 * device, ACCV_ELAUNCH if a launch fails.  The _host entries run the same operation sequence per pair on host memory and
 * block the calling thread. */
#define ACCV_PM_IDX_I64 1u
#define ACCV_PM_REVERSIBLE 2u
#define ACCV_PM_LABELS_I64 4u
#define ACCV_PM_CLOSED_I32 8u
#define ACCV_PM_CLOSED_I64 16u
/* the scalar parameters and optional operands, host memory, read during the call */
typedef struct accv_polyline_match_params {
    double class_weight, pts_weight;                  /* cost */
    double focal_alpha, focal_gamma, focal_eps, filler;
    double dir_eps;                                   /* loss */
    double avg_factor;                                /* the denominator of ACCV_FL_AVG_VALUE */
    long long pred_stride_b, pred_stride_q;           /* strides of pred_lines, in elements */
    int class_kind;                                   /* ACCV_MC_ONE_MINUS_PROB, ACCV_MC_NEG_PROB or ACCV_MC_FOCAL */
    int avg_mode;                                     /* ACCV_FL_AVG_NUM_POS, ACCV_FL_AVG_VALUE or ACCV_FL_AVG_DEVICE */
    int dir_loss;                                     /* 0: the direction term is not evaluated */
    const float* avg_factor_dev;                      /* the f32 scalar of ACCV_FL_AVG_DEVICE */
    const void* gt_closed;                            /* NULL or [B, G] */
} accv_polyline_match_params;
int accv_polyline_matching_cost(const void* pred_lines, const void* gt_lines, const void* scores, const void* gt_labels,
                                const long long* counts, int dtype, unsigned flags, long long B, long long Q, long long G,
                                long long P, long long D, long long C, long long scores_stride_b, long long scores_stride_q,
                                const accv_polyline_match_params* params, void* out, void* stream);
int accv_polyline_matching_cost_host(const void* pred_lines, const void* gt_lines, const void* scores, const void* gt_labels,
                                     const long long* counts, int dtype, unsigned flags, long long B, long long Q,
                                     long long G, long long P, long long D, long long C, long long scores_stride_b,
                                     long long scores_stride_q, const accv_polyline_match_params* params, void* out);
size_t accv_matched_polyline_loss_workspace_bytes(long long B, long long Q);
int accv_matched_polyline_loss(const void* pred_lines, const void* gt_lines, const void* pred_ind, const void* gt_ind,
                               const long long* counts, int dtype, unsigned flags, long long B, long long Q, long long G,
                               long long P, long long D, long long K, const accv_polyline_match_params* params, void* out,
                               double* out_denom, void* workspace, size_t workspace_bytes, void* stream);
int accv_matched_polyline_loss_bwd(const void* pred_lines, const void* gt_lines, const void* pred_ind, const void* gt_ind,
                                   const long long* counts, const void* grad_pts, const void* grad_dir, const double* denom,
                                   int dtype, unsigned flags, long long B, long long Q, long long G, long long P,
                                   long long D, long long K, const accv_polyline_match_params* params, void* grad_lines,
                                   void* stream);
int accv_matched_polyline_loss_host(const void* pred_lines, const void* gt_lines, const void* pred_ind, const void* gt_ind,
                                    const long long* counts, int dtype, unsigned flags, long long B, long long Q,
                                    long long G, long long P, long long D, long long K,
                                    const accv_polyline_match_params* params, void* out, double* out_denom);
int accv_matched_polyline_loss_bwd_host(const void* pred_lines, const void* gt_lines, const void* pred_ind,
                                        const void* gt_ind, const long long* counts, const void* grad_pts,
                                        const void* grad_dir, const double* denom, int dtype, unsigned flags, long long B,
                                        long long Q, long long G, long long P, long long D, long long K,
                                        const accv_polyline_match_params* params, void* grad_lines);

/* combine_data / split on device (batched_processing_py.py:410-423, ragged_batch.py:870-934):
 * unpack == 0: padded[i, j, :] = flat[offsets[i] + j, :] for j < sizes[i], zero bytes elsewhere;
 * unpack != 0: the inverse copy (flat <- padded, valid entries only).  offsets/sizes are device int64. */
int accv_ragged_pack(const void* flat, void* padded, const long long* offsets, const long long* sizes, long long batch,
                     long long width, long long row_bytes, int unpack, void* stream);

/* ------------------------------------------------------------------------------------------------ H3
 * Multi-tensor copier: pack planner, pinned arena, threaded staging + chunked host->device transfer, and a
 * device-side coalescing kernel.  Tensors, streams and events stay with the caller.
 */

/* Byte layout of the packed chunks — integer-exact counterpart of compute_pack_plan / layout_packed_offsets
 * (packages/multi_tensor_copier/accvlab/multi_tensor_copier/csrc/multi_tensor_copier.cpp:419-433, 513-549,
 * 553-590).  candidate[i] != 0 marks leaves that satisfy make_pack_candidate (:481-507: host tensor, target
 * is a GPU, contiguous, 0 < bytes <= 262144).  required_align = round_up(max(min_align, elem), elem); buckets
 * {16,8,4,2,1} are laid out in that order, insertion order inside a bucket; a new chunk starts when
 * offset + bytes > max_chunk_bytes and the chunk is not empty.  Fewer than 2 packed leaves => nothing is packed
 * (*out_num_chunks == 0, all offsets -1).  out_chunk_sizes must have room for n entries. Host arrays. */
int accv_mtc_plan(long long n, const long long* nbytes, const int* elem_size, const unsigned char* candidate,
                  long long min_align, long long max_chunk_bytes, long long* out_offset, long long* out_chunk,
                  long long* out_chunk_sizes, long long* out_num_chunks);

/* Pinned (page-locked) host buffers from a size-class cache over hipHostMalloc; replaces the per-call pinned
 * allocations of allocate_staging_buffers (multi_tensor_copier.cpp:597-641).  acquire returns NULL on failure. */
void* accv_pinned_acquire(size_t bytes);
void accv_pinned_release(void* ptr);
void accv_pinned_trim(void);
size_t accv_pinned_total_bytes(void);
int accv_mtc_worker_count(void);

/* DataLoader hook: host-only pack of `n_items` buffers into `dst` at the byte offsets of accv_mtc_plan
 * (single chunk).  Plain memcpy loop on the calling thread; makes no HIP call and uses no worker pool, so it is safe
 * inside forked DataLoader worker processes.  No reference counterpart (the reference packs in the consumer process,
 * fill_cpu_staging_buffers, multi_tensor_copier.cpp:647-679). */
int accv_mtc_pack_host(long long n_items, const void* const* src, const long long* nbytes, const long long* offset,
                       void* dst, long long dst_bytes);

/* fill_cpu_staging_buffers + enqueue_packed_transfer (multi_tensor_copier.cpp:647-679, 683-730): per chunk c,
 * memcpy src[i] -> staging[c] + offset[i] for i in order[item_begin[c] .. item_begin[c+1]) on up to `threads`
 * workers, then one hipMemcpyAsync(device[c] <- staging[c], chunk_bytes[c]) on `stream` (skipped when device[c]
 * is NULL).  All arrays are host memory; src/staging are host pointers, device[c] device pointers. */
int accv_mtc_stage_h2d(long long n_items, const void* const* src, const long long* nbytes, const long long* offset,
                       const long long* order, long long n_chunks, const long long* item_begin, void* const* staging,
                       void* const* device, const long long* chunk_bytes, void* stream, int threads);

/* The same staging + transfers on a native orchestration thread of the library (counterpart of the reference's
 * CopyThreadPool worker running schedule_copies, multi_tensor_copier.cpp:288-349, 863-883): the argument arrays are copied,
 * the job is queued and `*ticket_out` returned at once; no Python and no interpreter lock are involved in the work.
 * accv_mtc_async_wait(ticket) blocks until every transfer of the job has been ENQUEUED on `stream` (completion is the
 * caller's stream event) and returns the job's status; accv_mtc_async_poll(ticket) is 1 when it has finished, else 0.
 * A ticket is forgotten by the wait that returns its status.  device_index < 0 selects no device (a staging-only job whose
 * device[] entries are all NULL). */
int accv_mtc_stage_h2d_async(long long n_items, const void* const* src, const long long* nbytes, const long long* offset,
                             const long long* order, long long n_chunks, const long long* item_begin,
                             void* const* staging, void* const* device, const long long* chunk_bytes, void* stream,
                             int threads, int device_index, long long* ticket_out);
int accv_mtc_async_wait(long long ticket);
int accv_mtc_async_poll(long long ticket);
/* Orderly end of that thread (counterpart of ~CopyThreadPool joining its workers, multi_tensor_copier.cpp:300-312): runs
 * what is still queued, stops and joins; later accv_mtc_stage_h2d_async calls fail with ACCV_ERUNTIME.  Idempotent.  The
 * python package calls it from atexit, i.e. before the HIP runtime is torn down.  A forked child starts with fresh
 * (empty) pool / arena / orchestrator state: the parent's threads do not exist there. */
void accv_mtc_shutdown(void);
/* Number of tickets the orchestrator still remembers.  Bounded: a ticket is forgotten by the wait that returns its
 * status, and finished tickets nobody waited for are dropped once 1024 later jobs were submitted. */
long long accv_mtc_async_tickets_held(void);

/* One kernel that gathers (scatter == 0) many small device tensors into `packed`, or fans `packed` out again
 * (scatter != 0).  items: array of {const void* ptr; long long offset_in_packed; long long nbytes;} readable by
 * the device.  New component (the reference copies device tensors one by one, multi_tensor_copier.cpp:775-820). */
int accv_mtc_coalesce(const void* items, long long n_items, void* packed, int scatter, void* stream);

/* hipMemcpyAsync wrapper: kind 1 = H2D, 2 = D2H, 3 = D2D, anything else = default. */
int accv_memcpy_async(void* dst, const void* src, size_t bytes, int kind, void* stream);

/* ------------------------------------------------------------------------------------------------ lane_helpers
 * Batched polyline arc-length interpolation / lengths.  Replaces the four entry points of
 * packages/lane_helpers/ext_impl/polyline/src/polyline.cpp:101-398 (polyline_interpolation, _polyline_lengths and
 * their _var_size_batch forms; kernels include/polyline_kernels.cuh:390-455, semantics include/polyline_common.cuh
 * :58-163).  points [batch, max_points, dims], distances [batch, max_distances] (same dtype), optional per-polyline
 * counts (int32/int64; NULL = all valid).  out_points [batch, max_distances, dims] and/or out_lengths [batch] may be
 * NULL.  dtype: 0 f32, 1 f64, 2 f16, 3 bf16 (accumulation fp32, fp64 for f64).  relative != 0: distances are
 * fractions of the total length.  Polylines too long for LDS need accv_polyline_scratch_bytes() of device scratch. */
size_t accv_polyline_scratch_bytes(long long batch, int max_points, int dtype);
int accv_polyline_sample(const void* points, const void* distances, const void* point_counts, const void* dist_counts,
                         void* out_points, void* out_lengths, long long batch, int max_points, int max_distances,
                         int num_dims, int dtype, int counts_i64, int relative, void* scratch, size_t scratch_bytes,
                         void* stream);

/* The same operation on HOST memory (CPU tensors): counterpart of the reference's CPU implementation
 * (ext_impl/polyline/src/polyline_cpu.cpp:28-132): float32 / float64 only (dtype 0 / 1), double accumulation
 * (at::acc_type<dtype, false>), polylines split over up to `threads` host threads (0 = automatic).  No HIP call. */
int accv_polyline_sample_host(const void* points, const void* distances, const void* point_counts, const void* dist_counts,
                              void* out_points, void* out_lengths, long long batch, int max_points, int max_distances,
                              int num_dims, int dtype, int counts_i64, int relative, int threads);

/* The same sampler with one more output (float32 samples of 2-D points only): out_group_boxes f32[batch, ceil(Q/64), 4] =
 * (xmin, ymin, xmax, ymax) of every 64 consecutive samples of a polyline, NaN samples ignored, (+inf, +inf, -inf, -inf) for
 * a group without valid samples — what accv_draw_points_multiscale_f32 culls by (ACCV_HM_GROUP_BOXES_GIVEN saves its own
 * box launch).  NULL = plain accv_polyline_sample. */
int accv_polyline_sample_boxes(const void* points, const void* distances, const void* point_counts, const void* dist_counts,
                               void* out_points, void* out_lengths, float* out_group_boxes, long long batch, int max_points,
                               int max_distances, int num_dims, int dtype, int counts_i64, int relative, void* scratch,
                               size_t scratch_bytes, void* stream);

/* Backward of accv_polyline_sample (an extension: the reference's polyline operators have no gradient).  grad_out
 * [batch, max_distances, dims] (gradient of out_points) and grad_lengths [batch] (gradient of out_lengths) are in the points'
 * dtype, either may be NULL; writes grad_points [batch, max_points, dims] and / or grad_distances [batch, max_distances]
 * (either may be NULL) whole: zeros behind the counts, padded grad_out entries are not read.  Every query takes the segment
 * the forward's search took (same arithmetic); its gradient is the exact derivative of that branch: inside a segment of
 * length >= epsilon the interpolation, else the copied point.  Segments shorter than epsilon pass no length gradient;
 * polylines with 0 or 1 points give zero gradients.  Accumulation as the forward (f32 for f32 / f16 / bf16, f64 for f64;
 * the segment-length gradients are scanned in f64), through LDS / global float atomics: results may differ in the last
 * bits from run to run.  workspace: accv_polyline_grad_workspace_bytes(batch, max_points, max_distances, num_dims, dtype)
 * bytes of device memory with the same extents (max_distances = 0 when there are no distances).  No host synchronisation. */
size_t accv_polyline_grad_workspace_bytes(long long batch, int max_points, int max_distances, int num_dims, int dtype);
int accv_polyline_grad(const void* points, const void* distances, const void* point_counts, const void* dist_counts,
                       const void* grad_out, const void* grad_lengths, void* grad_points, void* grad_distances,
                       long long batch, int max_points, int max_distances, int num_dims, int dtype, int counts_i64,
                       int relative, void* workspace, size_t workspace_bytes, void* stream);
/* Its counterpart on HOST memory (accv_polyline_sample_host's backward): float32 / float64 only, double accumulation, up to
 * `threads` host threads (0 = automatic).  No HIP call. */
int accv_polyline_grad_host(const void* points, const void* distances, const void* point_counts, const void* dist_counts,
                            const void* grad_out, const void* grad_lengths, void* grad_points, void* grad_distances,
                            long long batch, int max_points, int max_distances, int num_dims, int dtype, int counts_i64,
                            int relative, int threads);

/* Streaming fill used by bench.py as the measured write-bandwidth ceiling (not part of the reference API). */
int accv_fill_f32(float* dst, size_t count, float value, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ACCV_HIP_H */
