"""Cases and the oracle of the visible-box selection tests (test_visible_boxes_cpu.py, test_visible_boxes_gpu.py).

The oracle is the canvas painter of the operator's definition (the docstring of accvlab.draw_heatmap.visible_bbox_mask),
written here in numpy from that text: it paints an H x W canvas per frame from far to near and looks which indices are
left.  The operator under test never paints a canvas, so the two share no code and no algorithm.
"""
import functools

import numpy as np
import torch

from accvlab.batching_helpers import RaggedBatch

F = np.float32
NAN, INF = float("nan"), float("inf")

# packages/dali_pipeline_framework/tests/processing_steps/visible_bbox_selector_test.py:62-80 of the reference, restated
REF_BOXES = [[10, 10, 40, 40], [10, 10, 25, 40], [25, 10, 40, 40], [60, 60, 80, 80], [50, 50, 90, 90], [0, 0, 5, 5],
             [10, 10, 11, 100], [10, 10, 100, 11], [110, 120, 200, 300], [110, 10, 150, 60], [130, 5, 150, 70]]
REF_DEPTHS = [5.0, 1.0, 2.0, 4.0, 1.5, 0.5, 0.1, 0.2, 0.3, 0.3, 0.3]
REF_HW = (100, 200)                                              # :42
REF_OCCLUSION = [0, 1, 1, 0, 1, 1, 1, 1, 0, 1, 1]                # :169-184 with the occlusion check alone
REF_SIZE = [1, 1, 1, 1, 1, 1, 0, 0, 0, 1, 1]                     # minimum_size = 2: box 8 is clipped to height 0


# ---------------------------------------------------------------------------------------------------------------- oracle
def _above(dj, j, di, i):
    """box j lies above box i (step 5 of the definition)"""
    nj, ni = np.isnan(dj), np.isnan(di)
    if nj != ni:
        return bool(nj)
    if nj:
        return j > i
    return bool(dj < di) or (bool(dj == di) and j > i)


def _rect(box, H, W, shrink):
    """the painted rectangle (x0, y0, x1, y1) of steps 1 to 4, None when the box paints nothing"""
    box = np.asarray(box, F)
    if np.isnan(box).any():
        return None
    out = []
    for a, b, E in ((box[0], box[2], W), (box[1], box[3], H)):
        mn, mx = (a, b) if a < b else (b, a)
        lo, hi = (np.ceil(mn), np.floor(mx)) if shrink else (np.floor(mn), np.ceil(mx))
        lo, hi = (int(np.clip(v, F(-1), F(E) + F(1))) for v in (lo, hi))
        if lo > E or hi < 0:
            return None
        out.append((max(lo, 0), min(hi, E)))
    (x0, x1), (y0, y1) = out
    return (x0, y0, x1, y1) if x0 < x1 and y0 < y1 else None


def oracle_frame(boxes, depths, hw, *, check_occlusion=True, minimum_size=None, shrink_to_int=False):
    """bool [n] of one frame by painting an H x W canvas"""
    boxes = np.asarray(boxes, F).reshape(-1, 4)
    n, (H, W) = len(boxes), (int(np.clip(v, 0, 1 << 24)) for v in hw)
    res = np.ones(n, bool)
    if check_occlusion:
        depths = np.asarray(depths, F)
        order = sorted(range(n), key=functools.cmp_to_key(lambda i, j: 1 if _above(depths[i], i, depths[j], j) else -1))
        canvas = np.full((H, W), -1, np.int32)
        for i in order:                                          # far to near, the last painted on top
            r = _rect(boxes[i], H, W, shrink_to_int)
            if r is not None:
                canvas[r[1]:r[3], r[0]:r[2]] = i
        seen = np.unique(canvas)
        res[:] = False
        res[seen[seen >= 0]] = True
    if minimum_size is not None:
        with np.errstate(invalid="ignore"):
            dx = np.abs(np.clip(boxes[:, 2], F(0), F(W)) - np.clip(boxes[:, 0], F(0), F(W)))
            dy = np.abs(np.clip(boxes[:, 3], F(0), F(H)) - np.clip(boxes[:, 1], F(0), F(H)))
            res &= (dx >= F(minimum_size)) & (dy >= F(minimum_size))
    return res


def oracle(frames, G, **kw):
    """bool tensor [B, G] of a list of (boxes, depths, hw) frames; padding False"""
    out = torch.zeros((len(frames), G), dtype=torch.bool)
    for b, (boxes, depths, hw) in enumerate(frames):
        n = len(boxes)
        if n:
            out[b, :n] = torch.from_numpy(oracle_frame(boxes, depths, hw, **kw))
    return out


# --------------------------------------------------------------------------------------------------------------- batches
def batch(frames, G=None, device="cpu", hostile_padding=True, size_dtype=torch.int64, hw_dtype=torch.int32):
    """(bboxes RaggedBatch [B, G, 4], depths RaggedBatch [B, G], image_hw tensor [B, 2]) of a list of
    (boxes, depths, hw) frames.  With hostile_padding the slots behind a frame's boxes hold NaN, 1e30 and boxes that cover
    the whole image, at depth -1, which would put them on top of every real box."""
    B = len(frames)
    G = max([len(f[0]) for f in frames] + [0]) if G is None else G
    boxes = torch.zeros((B, G, 4), dtype=torch.float32)
    depths = torch.zeros((B, G), dtype=torch.float32)
    if hostile_padding:
        fill = torch.tensor([[NAN, NAN, NAN, NAN], [-1e30, -1e30, 1e30, 1e30], [-5.0, -5.0, 4e7, 4e7], [0.0, 0.0, 1e30, NAN]])
        boxes[:] = fill[torch.arange(G) % 4]
        depths[:] = -1.0
    for b, (bx, dp, _) in enumerate(frames):
        n = len(bx)
        if n:
            boxes[b, :n] = torch.as_tensor(np.asarray(bx, F).reshape(-1, 4))
            depths[b, :n] = torch.as_tensor(np.asarray(dp, F))
    sizes = torch.tensor([len(f[0]) for f in frames], dtype=size_dtype)
    hw = torch.tensor([list(f[2]) for f in frames], dtype=hw_dtype).reshape(B, 2)
    return (RaggedBatch(boxes.to(device), sample_sizes=sizes.to(device)),
            RaggedBatch(depths.to(device), sample_sizes=sizes.to(device)), hw.to(device))


def random_frame(rng, n, hw, depth_values=8):
    """n boxes on the half-integer lattice (coinciding edges), depths from a small set (ties), a fifth flipped, a few
    reaching over the image border; sizes from a few pixels to most of the image, so that both outcomes are common"""
    H, W = hw
    cx, cy = rng.integers(-4, 2 * W + 5, n) / 2.0, rng.integers(-4, 2 * H + 5, n) / 2.0
    scale = rng.choice([0.08, 0.2, 0.45], n)
    w = np.maximum(rng.integers(0, 2 * W + 1, n) * scale, 0.0).round() / 2.0
    h = np.maximum(rng.integers(0, 2 * H + 1, n) * scale, 0.0).round() / 2.0
    boxes = np.stack([cx - w, cy - h, cx + w, cy + h], 1).astype(F)
    flip = rng.random(n) < 0.2
    boxes[flip] = boxes[flip][:, [2, 3, 0, 1]]
    depths = rng.integers(0, depth_values, n).astype(F) / 2
    return boxes, depths, hw


PARTITION_SIZES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256)


def partition_frames(seed=7, hw=(40, 56)):
    rng = np.random.default_rng(seed)
    return [random_frame(rng, n, hw, depth_values=24) for n in PARTITION_SIZES]


def sweep_frames(seed, count=24):
    rng = np.random.default_rng(seed)
    frames = []
    for _ in range(count):
        hw = (int(rng.integers(1, 65)), int(rng.integers(1, 97)))
        frames.append(random_frame(rng, int(rng.integers(0, 49)), hw))
    return frames


# ----------------------------------------------------------------------------------------------------- geometry edges
# name -> (boxes, depths, hw, expected with the corners rounded outwards, expected with shrink_to_int), occlusion check
# alone, on a 12 x 20 image unless the case is about the image size.  The expectations are worked by hand; the tests also
# hold them against the oracle.
HW = (12, 20)
GEOMETRY = {
    "identical_boxes_equal_depth": ([[2, 2, 8, 8]] * 3, [1, 1, 1], HW, [0, 0, 1], [0, 0, 1]),
    "negative_zero_ties_with_zero": ([[2, 2, 8, 8]] * 3, [0.0, -0.0, 0.0], HW, [0, 0, 1], [0, 0, 1]),
    "negative_zero_first": ([[2, 2, 8, 8]] * 2, [-0.0, 0.0], HW, [0, 1], [0, 1]),
    "nested_chain_near_inside_far": ([[1, 1, 11, 11], [2, 2, 10, 10], [3, 3, 9, 9]], [3, 2, 1], HW, [1, 1, 1], [1, 1, 1]),
    "nested_chain_far_inside_near": ([[1, 1, 11, 11], [2, 2, 10, 10], [3, 3, 9, 9]], [1, 2, 3], HW, [1, 0, 0], [1, 0, 0]),
    "union_of_two_covers": ([[4, 2, 12, 8], [4, 2, 8, 8], [8, 2, 12, 8]], [5, 1, 2], HW, [0, 1, 1], [0, 1, 1]),
    "union_of_two_with_a_gap": ([[4, 2, 12, 8], [4, 2, 8, 8], [9, 2, 12, 8]], [5, 1, 2], HW, [1, 1, 1], [1, 1, 1]),
    "union_of_four_covers": ([[4, 2, 12, 10], [4, 2, 8, 6], [8, 2, 12, 6], [4, 6, 8, 10], [8, 6, 12, 10]], [9, 1, 2, 3, 4], HW,
                             [0, 1, 1, 1, 1], [0, 1, 1, 1, 1]),
    "union_of_four_with_a_gap": ([[4, 2, 12, 10], [4, 2, 8, 6], [8, 2, 12, 6], [4, 6, 8, 10], [8, 7, 12, 10]], [9, 1, 2, 3, 4], HW,
                                 [1, 1, 1, 1, 1], [1, 1, 1, 1, 1]),
    "flipped_corners": ([[12, 8, 4, 2], [4, 8, 12, 2], [13, 1, 3, 9]], [5, 1, 0.5], HW, [0, 0, 1], [0, 0, 1]),
    # the far box ends at x = 8.4: rounded outwards it shows the column [8, 9) beside the near box, shrunk it ends at 8
    "fraction_rounded_outwards_or_inwards": ([[4, 2, 8.4, 8], [4, 2, 8, 8]], [5, 1], HW, [1, 1], [0, 1]),
    "sliver_of_width_0p4": ([[5.3, 2, 5.7, 8]], [1], HW, [1], [0]),
    "partly_outside": ([[-5, -5, 3, 3], [15, 8, 30, 30]], [1, 2], HW, [1, 1], [1, 1]),
    "outside_on_each_side": ([[-9, 2, -2, 8], [22, 2, 30, 8], [2, -9, 8, -2], [2, 14, 8, 20]], [1, 2, 3, 4], HW,
                             [0, 0, 0, 0], [0, 0, 0, 0]),
    "min_x_equals_w_and_max_x_equals_0": ([[20, 2, 25, 8], [-5, 2, 0, 8], [2, 12, 8, 15], [2, -4, 8, 0]], [1, 2, 3, 4], HW,
                                          [0, 0, 0, 0], [0, 0, 0, 0]),
    "zero_area": ([[5, 5, 5, 9], [3, 4, 9, 4], [6, 6, 6, 6]], [1, 2, 3], HW, [0, 0, 0], [0, 0, 0]),
    "nan_coordinate_paints_nothing": ([[2, 2, 8, 8], [NAN, 0, 20, 12], [0, 0, 20, NAN]], [5, 1, 1], HW, [1, 0, 0], [1, 0, 0]),
    "nan_depth_lies_on_top": ([[2, 2, 8, 8], [0, 0, 20, 12], [3, 3, 5, 5]], [-INF, NAN, 1], HW, [0, 1, 0], [0, 1, 0]),
    "two_nan_depths_tie": ([[2, 2, 8, 8], [2, 2, 8, 8]], [NAN, NAN], HW, [0, 1], [0, 1]),
    "infinite_and_huge_coordinates": ([[-INF, -INF, INF, INF], [-1e30, 2, 1e30, 4], [5, 5, 6, 6], [INF, 0, INF, 12], [1e30, 0, 2e30, 12]],
                                      [9, 8, 7, 1, 1], HW, [1, 1, 1, 0, 0], [1, 1, 1, 0, 0]),
    "height_zero": ([[2, 2, 8, 8], [0, 0, 20, 0]], [1, 2], (0, 20), [0, 0], [0, 0]),
    "width_zero": ([[2, 2, 8, 8], [0, 0, 0, 12]], [1, 2], (12, 0), [0, 0], [0, 0]),
}


def geometry_frames(names=None):
    return [(GEOMETRY[k][0], GEOMETRY[k][1], GEOMETRY[k][2]) for k in (names or sorted(GEOMETRY))]


def geometry_expected(shrink, G, names=None):
    names = names or sorted(GEOMETRY)
    out = torch.zeros((len(names), G), dtype=torch.bool)
    for b, k in enumerate(names):
        want = GEOMETRY[k][4 if shrink else 3]
        out[b, :len(want)] = torch.tensor(want, dtype=torch.bool)
    return out


# two frames that differ only in their image_hw row: the box is inside the first image and outside the second
TWO_SIZES = [([[30, 30, 40, 40], [2, 2, 8, 8]], [1, 2], (50, 50)), ([[30, 30, 40, 40], [2, 2, 8, 8]], [1, 2], (12, 20))]
TWO_SIZES_EXPECTED = [[1, 1], [0, 1]]

# H = W = 2^24 with a handful of boxes: nothing of the size of the image can be allocated
E24 = 1 << 24
HUGE = ([[0, 0, E24, E24], [0, 0, E24 - 1, E24], [E24 - 1, 0, E24, E24 - 1], [100, 100, 200, 200], [E24, 5, E24 + 2, 9],
         [E24 - 1, E24 - 1, E24, E24]], [9, 1, 1, 5, 1, 0.5], (E24, E24))
# box 0 shows only through the pixel (E24 - 1, E24 - 1) that boxes 1 and 2 leave, and box 5 takes exactly that pixel
HUGE_EXPECTED = [0, 1, 1, 0, 0, 1]
HUGE_WITHOUT_LAST_EXPECTED = [1, 1, 1, 0, 0]


# ---------------------------------------------------------------------------------------------------------------- running
def run(op, frames, device="cpu", G=None, hw_as="tensor", **kw):
    """the operator's mask [B, G] (on the CPU) of a list of frames, padding slots checked on the way"""
    boxes, depths, hw = batch(frames, G, device, hw_dtype=torch.int64 if hw_as == "int64" else torch.int32)
    if hw_as == "tuple":
        assert len({tuple(f[2]) for f in frames}) == 1
        hw = tuple(frames[0][2])
    got = op(boxes, depths if kw.get("check_occlusion", True) else None, image_hw=hw, **kw)
    assert got.tensor.dtype == torch.bool and got.tensor.shape == boxes.tensor.shape[:2]
    assert got.tensor.device == boxes.tensor.device and got.sample_sizes is boxes.sample_sizes
    mask = got.tensor.cpu()
    for b, f in enumerate(frames):
        assert not bool(mask[b, len(f[0]):].any()), f"frame {b}: a padding slot came out True"
    return mask


def all_case_sets():
    """(name, frames, keyword sets) of every case family of the tests, for the path comparisons"""
    both = (dict(), dict(shrink_to_int=True), dict(minimum_size=2), dict(check_occlusion=False, minimum_size=1.5))
    ref = [(REF_BOXES, REF_DEPTHS, REF_HW)]
    return [("reference", ref, both), ("partition", partition_frames(), both[:3]), ("geometry", geometry_frames(), both),
            ("two_sizes", TWO_SIZES, both[:2]), ("sweep", sweep_frames(3), both), ("huge", [HUGE], both[:2])]
