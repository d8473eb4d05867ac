"""The prediction side of a CenterPoint head, from the network's outputs to detections, for the six nuScenes tasks:

    heatmap_peaks        the K strongest cells of each task's heat-map LOGITS (no sigmoid pass over the map): two launches
    center_point_decode  peaks + regression heads of every task -> filtered, circle-NMS'd, compacted boxes: ONE launch

`fused_decode` is that path; nothing in it synchronises with the host.  `composed_decode` is what it replaces, written
after mmdet3d's CenterPointBBoxCoder.decode and the `circle` branch of CenterHead.get_bboxes: per task sigmoid, topk, five
gathers, exp / atan2 / the affine map, two masks, and per frame a boolean index, the centres to the host, the circle NMS
there and the kept indices back.  Both print the same detections.

    python3 examples/centerpoint_decode.py [--nms {circle,rotate}]

`--nms rotate` shows the other branch of CenterHead.get_bboxes: the decode runs without NMS and `rotated_nms_bev` (rotated
BEV-IoU NMS, mmdet3d's nms_bev over mmcv's nms_rotated) follows it, again for every task in one launch and without a host
round trip; it is compared with the library's own host entry on a copy of the decode's output.
"""
from __future__ import annotations

import argparse
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "accv-lab_amd"))   # run from a checkout

import numpy as np
import torch

from accvlab.batching_helpers import RaggedBatch
from accvlab.draw_heatmap import CenterPointDetections, center_point_decode, gather_at_centers, heatmap_peaks, rotated_nms_bev

TASKS = ((0,), (1, 2), (3, 4), (5,), (6, 7), (8, 9))            # the six nuScenes tasks over ten classes
MIN_RADIUS = [4, 12, 10, 1, 0.85, 0.175]                        # mmdet3d's nuScenes test_cfg
CFG = dict(pc_range=[-51.2, -51.2], voxel_size=[0.2, 0.2], out_size_factor=4)
TEST = dict(score_threshold=0.1, post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], nms_threshold=MIN_RADIUS, post_max_size=83)
ROTATE = dict(iou_threshold=0.2, pre_max_size=1000, post_max_size=83)   # mmdet3d's nuScenes test_cfg of the `rotate` branch
H = W = 128
K = 500


def make_heads(batch: int, device, seed: int = 1):
    """what the network would predict: per task the heat-map logits and the five regression heads (reg, height, dim, rot, vel)"""
    g = torch.Generator().manual_seed(seed)
    logits, heads = [], []
    for ids in TASKS:
        logits.append((torch.randn(batch, len(ids), H, W, generator=g) - 3.0).to(device))
        ang = (torch.rand(batch, 1, H, W, generator=g) * 2 - 1) * math.pi
        heads.append([t.contiguous().to(device) for t in (
            torch.rand(batch, 2, H, W, generator=g), torch.rand(batch, 1, H, W, generator=g) * 8 - 5,
            torch.rand(batch, 3, H, W, generator=g) * 3 - 1, torch.cat([ang.sin(), ang.cos()], 1),
            torch.rand(batch, 2, H, W, generator=g) * 10 - 5)])
    return logits, heads


def fused_decode(logits, heads):
    peaks = [heatmap_peaks(lg, K, kernel=1) for lg in logits]                 # ranks the logits: sigmoid is monotone
    return peaks, center_point_decode(peaks, heads, TASKS, **CFG, scores_are_logits=True, **TEST)


def rotate_decode(logits, heads):
    """the `rotate` branch: the decode without NMS, then the rotated NMS of every task in one launch"""
    peaks = [heatmap_peaks(lg, K, kernel=1) for lg in logits]
    test = dict(TEST, nms_threshold=None, post_max_size=None)
    dets = center_point_decode(peaks, heads, TASKS, **CFG, scores_are_logits=True, **test)
    return peaks, dets, rotated_nms_bev(dets, ROTATE["iou_threshold"], pre_max_size=ROTATE["pre_max_size"], post_max_size=ROTATE["post_max_size"])


def circle_nms(xy, thresh, post_max_size):
    """mmdet3d's circle_nms on host centres in descending score order"""
    dead, keep = np.zeros(len(xy), bool), []
    for i in range(len(xy)):
        if dead[i]:
            continue
        keep.append(i)
        if len(keep) >= post_max_size:
            break
        d = xy[i + 1:] - xy[i]
        dead[i + 1:] |= (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) <= thresh
    return keep


def composed_decode(logits, heads):
    out = []
    rng = torch.tensor(TEST["post_center_range"], device=logits[0].device)
    for t, (lg, hd) in enumerate(zip(logits, heads)):
        batch = lg.shape[0]
        scores, inds = lg.sigmoid().view(batch, -1).topk(K)
        clses, inds = inds // (H * W), inds % (H * W)
        reg, hei, dim, rot, vel = (f.view(batch, f.shape[1], -1).permute(0, 2, 1).gather(1, inds[..., None].expand(-1, -1, f.shape[1]))
                                   for f in hd)
        xs = ((inds % W).float() + reg[..., 0]) * CFG["out_size_factor"] * CFG["voxel_size"][0] + CFG["pc_range"][0]
        ys = ((inds // W).float() + reg[..., 1]) * CFG["out_size_factor"] * CFG["voxel_size"][1] + CFG["pc_range"][1]
        boxes = torch.cat([xs[..., None], ys[..., None], hei, dim.exp(), torch.atan2(rot[..., 0:1], rot[..., 1:2]), vel], -1)
        mask = (scores > TEST["score_threshold"]) & (boxes[..., :3] >= rng[:3]).all(-1) & (boxes[..., :3] <= rng[3:]).all(-1)
        ids = torch.tensor(TASKS[t], device=lg.device)
        frames = []
        for b in range(batch):
            bx, sc, lb = boxes[b][mask[b]], scores[b][mask[b]], ids[clses[b][mask[b]]]
            keep = torch.tensor(circle_nms(bx[:, :2].cpu().numpy(), MIN_RADIUS[t], TEST["post_max_size"]), dtype=torch.long, device=lg.device)
            frames.append((bx[keep], sc[keep], lb[keep]))
        out.append(frames)
    return out


def main_rotate(logits, heads):
    peaks, before, dets = rotate_decode(logits, heads)
    on_host = []                                                                       # the same operator on host copies
    for d in before:
        sizes = d.boxes.sample_sizes.cpu()
        on_host.append(CenterPointDetections(*(RaggedBatch(x.tensor.cpu(), sample_sizes=sizes) for x in d)))
    ref = rotated_nms_bev(on_host, ROTATE["iou_threshold"], pre_max_size=ROTATE["pre_max_size"], post_max_size=ROTATE["post_max_size"])
    for t, (d, r, b4) in enumerate(zip(dets, ref, before)):
        for b in range(d.boxes.tensor.shape[0]):
            n = int(d.boxes.sample_sizes[b])
            same = n == int(r.boxes.sample_sizes[b]) and torch.equal(d.source.tensor[b].cpu(), r.source.tensor[b])
            print(f"task {t} frame {b}: {int(b4.boxes.sample_sizes[b])} decoded, {n} after rotated NMS, equal to the host entry {same}, "
                  f"best score {float(d.scores.tensor[b, 0]):.3f} from peak rank {int(d.source.tensor[b, 0])}")
    d = dets[0]
    cells = peaks[0].indices.gather(1, d.source.tensor.clamp(min=0).long())
    rows = gather_at_centers(heads[0], cells)
    print("rows of task 0 for a loss on the detections:", tuple(rows.shape))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nms", choices=("circle", "rotate"), default="circle")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this example runs heatmap_peaks, which needs a GPU")
    dev = torch.device("cuda", 0)
    logits, heads = make_heads(2, dev)
    if args.nms == "rotate":
        return main_rotate(logits, heads)
    peaks, dets = fused_decode(logits, heads)
    ref = composed_decode(logits, heads)
    for t, (d, frames) in enumerate(zip(dets, ref)):
        for b, (bx, sc, lb) in enumerate(frames):
            n = int(d.boxes.sample_sizes[b])
            same = n == len(bx) and bool((d.labels.tensor[b, :n] == lb).all())
            err = float((d.boxes.tensor[b, :n] - bx).abs().max()) if same and n else float("nan")
            print(f"task {t} frame {b}: {n} detections (composition {len(bx)}), labels equal {same}, boxes max abs diff {err:.2e}, "
                  f"best score {float(d.scores.tensor[b, 0]):.3f} from peak rank {int(d.source.tensor[b, 0])}")
    # training through the selected values: gather them again at the cells the detections came from
    d = dets[0]
    cells = peaks[0].indices.gather(1, d.source.tensor.clamp(min=0).long())
    rows = gather_at_centers(heads[0], cells)
    print("rows of task 0 for a loss on the detections:", tuple(rows.shape))


if __name__ == "__main__":
    main()
