"""The prediction side of a CenterNet-style camera head, from the network's outputs to boxes in the SOURCE images:

    heatmap_peaks        the K strongest cells of the heat-map LOGITS (no sigmoid pass over the map): two launches
    box_heatmap_decode   peaks + offset and size maps -> filtered, IoU-NMS'd, compacted xyxy boxes, taken back through the
                         matrix the images were prepared with: ONE launch

`fused_decode` is that path; nothing in it synchronises with the host.  The matrices are those of `sample_image_transforms`,
the ones `prepare_images` warped the images with and `camera_augment_boxes` the annotations: the decoder applies their
inverse, so the detections land in the pixels of the camera images.  `composed_decode` is what it replaces, written after
mmdet's CenterNetHead._decode_heatmap and batched_nms: sigmoid, topk, two gathers, a dozen element-wise launches, and per
frame a boolean index, the boxes to the host, a greedy NMS loop there (the ROCm build of torch has no torchvision) and the
kept indices back.  Both print the same detections.

    python3 examples/camera_decode_step.py [--samples 2] [--cameras 6]
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "accv-lab_amd"))   # run from a checkout

import numpy as np
import torch

from accvlab.draw_heatmap import box_heatmap_decode, heatmap_peaks
from accvlab.image_prep import NonUniformScaling, ShiftToAlignWithOriginalImageBorder, UniformScaling, padded_hw, sample_image_transforms

CATEGORIES = 10
STRIDE = 4
K = 100
TEST = dict(score_threshold=0.1, iou_threshold=0.5, post_max_size=50)


def make_heads(frames: int, map_hw, device, seed: int = 1):
    """what the network would predict: the heat-map logits, the centre offsets and the sizes (h, w) in map pixels"""
    g = torch.Generator().manual_seed(seed)
    Hm, Wm = map_hw
    logits = (torch.randn(frames, CATEGORIES, Hm, Wm, generator=g) - 3.0).to(device)
    offset = torch.rand(frames, 2, Hm, Wm, generator=g).to(device)
    size = (2.0 + 20.0 * torch.rand(frames, 2, Hm, Wm, generator=g)).to(device)
    return logits, [offset, size]


def fused_decode(logits, heads, image_hw, matrices):
    peaks = heatmap_peaks(logits, K, kernel=1)                                 # ranks the logits: sigmoid is monotone
    return box_heatmap_decode(peaks, heads, image_hw=image_hw, image_matrices=matrices, scores_are_logits=True, **TEST)


def greedy_nms(boxes, labels, thresh, post_max_size):
    """greedy IoU NMS on host boxes in descending score order, class-aware"""
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    dead, keep = np.zeros(len(boxes), bool), []
    for i in range(len(boxes)):
        if dead[i]:
            continue
        keep.append(i)
        if len(keep) >= post_max_size:
            break
        rest = boxes[i + 1:]
        iw = np.clip(np.minimum(boxes[i, 2], rest[:, 2]) - np.maximum(boxes[i, 0], rest[:, 0]), 0, None)
        ih = np.clip(np.minimum(boxes[i, 3], rest[:, 3]) - np.maximum(boxes[i, 1], rest[:, 1]), 0, None)
        inter = iw * ih
        with np.errstate(invalid="ignore", divide="ignore"):
            dead[i + 1:] |= (inter / (area[i] + area[i + 1:] - inter) > thresh) & (labels[i + 1:] == labels[i])
    return keep


def composed_decode(logits, heads, image_hw, matrices):
    frames, _, Hm, Wm = logits.shape
    scores, inds = logits.sigmoid().view(frames, -1).topk(K)
    clses, inds = inds // (Hm * Wm), inds % (Hm * Wm)
    off, hw = (f.view(frames, 2, -1).permute(0, 2, 1).gather(1, inds[..., None].expand(-1, -1, 2)) for f in heads)
    cx, cy = (inds % Wm).float() + off[..., 0], (inds // Wm).float() + off[..., 1]
    ux, uy = image_hw[1] / Wm, image_hw[0] / Hm
    boxes = torch.stack([((cx - 0.5 * hw[..., 1]) * ux).clamp(0, image_hw[1]), ((cy - 0.5 * hw[..., 0]) * uy).clamp(0, image_hw[0]),
                         ((cx + 0.5 * hw[..., 1]) * ux).clamp(0, image_hw[1]), ((cy + 0.5 * hw[..., 0]) * uy).clamp(0, image_hw[0])], -1)
    mask = scores > TEST["score_threshold"]
    out = []
    for f in range(frames):
        bx, sc, lb = boxes[f][mask[f]], scores[f][mask[f]], clses[f][mask[f]]
        keep = torch.tensor(greedy_nms(bx.cpu().numpy(), lb.cpu().numpy(), TEST["iou_threshold"], TEST["post_max_size"]),
                            dtype=torch.long, device=logits.device)
        bx = bx[keep]
        # back to the source image: the inverse of the frame's 2 x 3 matrix, corner by corner, then the corners in order
        A, t = matrices[f, :, :2], matrices[f, :, 2]
        corners = torch.linalg.solve(A, (bx.view(-1, 2) - t).t()).t().view(-1, 2, 2)
        out.append((torch.cat([corners.min(1).values, corners.max(1).values], 1), sc[keep], lb[keep]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=2)
    ap.add_argument("--cameras", type=int, default=6)
    ap.add_argument("--source", type=int, nargs=2, default=(900, 1600))
    ap.add_argument("--output", type=int, nargs=2, default=(256, 704))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this example runs heatmap_peaks, which needs a GPU")
    dev = torch.device("cuda", 0)
    source_hw, output_hw = tuple(args.source), tuple(args.output)
    frames = args.samples * args.cameras
    steps = [NonUniformScaling(0.5, (-1.0, 1.0)),                       # the horizontal flip
             UniformScaling(1.0, 0.9, 1.1), ShiftToAlignWithOriginalImageBorder(1.0, "bottom")]
    matrices = sample_image_transforms(args.samples, args.cameras, steps, source_hw=source_hw, output_hw=output_hw, mode="crop",
                                       anchor="bottom_or_right", generator=torch.Generator().manual_seed(0)).to(dev)
    hw = padded_hw(output_hw, 32)                                       # what the network saw
    logits, heads = make_heads(frames, (hw[0] // STRIDE, hw[1] // STRIDE), dev)

    dets = fused_decode(logits, heads, hw, matrices)
    ref = composed_decode(logits, heads, hw, matrices)
    for f, (bx, sc, lb) in enumerate(ref):
        n = int(dets.boxes.sample_sizes[f])
        same = n == len(bx) and bool((dets.labels.tensor[f, :n] == lb).all())
        err = float((dets.boxes.tensor[f, :n] - bx).abs().max()) if same and n else float("nan")
        flipped = float(matrices[f, 0, 0]) < 0
        print(f"frame {f}{' (flipped)' if flipped else ''}: {n} detections (composition {len(bx)}), labels equal {same}, boxes max abs "
              f"diff {err:.2e} px of {source_hw[1]}, best score {float(dets.scores.tensor[f, 0]):.3f} from peak rank "
              f"{int(dets.source.tensor[f, 0])}, box {[round(v, 1) for v in dets.boxes.tensor[f, 0].tolist()]}")


if __name__ == "__main__":
    main()
