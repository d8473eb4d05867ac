#!/usr/bin/env python3
"""Host cost per call of the detection decoders on CPU tensors at their smallest legal shapes (one frame, K or N = 2, maps
[1, c, 2, 2]), where the library's host entry does next to nothing and the loop time is the Python intake and output layer.

  one run     scripts/detection_intake_host_cost.py --package DIR      DIR holds the accvlab package (default: this tree's);
                                                                        prints one JSON line of us per call, 2000 calls each
  the calls   scripts/detection_intake_host_cost.py --package DIR --count    function calls (Python and C) per operator call
  the A/B     scripts/detection_intake_host_cost.py --against DIR      alternates DIR (the parent's tree, exported with its
                                                                        library) and this tree, three fresh processes each, and
                                                                        prints both sets, the medians and the parent's spread

gather_at_centers / center_regression_loss have no CPU path and are not timed.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "accv-lab_amd")
CALLS, WARMUP, RUNS = 2000, 200, 3


def one_run(package, count=False):
    sys.path.insert(0, package)
    import torch
    from accvlab.batching_helpers import RaggedBatch
    from accvlab.draw_heatmap import (BoxDetections, CenterPointDetections, HeatmapPeaks, box_heatmap_decode, center_point_decode,
                                      nms_boxes, query_box_decode_2d, query_box_decode_3d, rotated_nms_bev)
    import accvlab.draw_heatmap as dh
    assert dh.__file__.startswith(os.path.abspath(package) + os.sep), dh.__file__
    torch.set_num_threads(1)
    i64, i32 = torch.int64, torch.int32
    idx = torch.zeros((1, 2), dtype=i64)
    peaks = HeatmapPeaks(torch.zeros((1, 2)), idx, idx.clone(), idx.clone(), idx.clone())
    maps8, maps4 = torch.zeros((1, 8, 2, 2)), torch.zeros((1, 4, 2, 2))
    sizes = torch.full((1,), 2, dtype=i64)
    members = (torch.zeros((1, 2)), torch.zeros((1, 2), dtype=i64), torch.zeros((1, 2), dtype=i32))
    d3 = CenterPointDetections(*(RaggedBatch(x, sample_sizes=sizes) for x in (torch.zeros((1, 2, 7)),) + members))
    d2 = BoxDetections(*(RaggedBatch(x, sample_sizes=sizes) for x in (torch.zeros((1, 2, 4)),) + members + (torch.zeros((1, 2, 0)),)))
    cls, rows8, rows4 = torch.zeros((1, 2, 1)), torch.zeros((1, 2, 8)), torch.zeros((1, 2, 4))
    ops = {
        "center_point_decode": lambda: center_point_decode(peaks, maps8, [[0]], pc_range=(0.0, 0.0), voxel_size=(1.0, 1.0),
                                                           out_size_factor=1, score_threshold=0.1, nms_threshold=0.5, post_max_size=2),
        "rotated_nms_bev": lambda: rotated_nms_bev(d3, 0.5, pre_max_size=2, post_max_size=2),
        "box_heatmap_decode": lambda: box_heatmap_decode(peaks, maps4, image_hw=(2, 2), score_threshold=0.1, iou_threshold=0.5,
                                                         post_max_size=2),
        "nms_boxes": lambda: nms_boxes(d2, 0.5, pre_max_size=2, post_max_size=2),
        "query_box_decode_3d": lambda: query_box_decode_3d(cls, rows8, 1, score_threshold=0.1),
        "query_box_decode_2d": lambda: query_box_decode_2d(cls, rows4, 1, image_hw=(2, 2), score_threshold=0.1),
    }
    out = {}
    for name, fn in ops.items():
        for _ in range(WARMUP):
            fn()
        if count:   # the function calls (Python and C) one operator call makes: what a timer on a shared machine cannot resolve
            import cProfile
            import pstats
            prof = cProfile.Profile()
            prof.runcall(fn)
            out[name] = pstats.Stats(prof).total_calls
            continue
        t0 = time.perf_counter()
        for _ in range(CALLS):
            fn()
        out[name] = round((time.perf_counter() - t0) / CALLS * 1e6, 2)
    print(json.dumps(out))


def against(parent):
    runs = {"parent": [], "this": []}
    for _ in range(RUNS):
        for side, package in (("parent", parent), ("this", HERE)):
            line = subprocess.run([sys.executable, os.path.abspath(__file__), "--package", package], check=True, capture_output=True,
                                  text=True).stdout.strip().splitlines()[-1]
            print(f"{side:6s} {line}", flush=True)
            runs[side].append(json.loads(line))
    print(f"\nus per call, median of {RUNS} runs of {CALLS} calls; the margin is the parent's own spread (max - min of its runs)")
    print(f"{'operator':22s} {'parent':>8s} {'this':>8s} {'this - parent':>14s} {'parent spread':>14s}  within")
    ok = True
    for name in runs["parent"][0]:
        p, t = [r[name] for r in runs["parent"]], [r[name] for r in runs["this"]]
        mp, mt, spread = statistics.median(p), statistics.median(t), max(p) - min(p)
        inside = abs(mt - mp) <= spread
        ok = ok and inside
        print(f"{name:22s} {mp:8.2f} {mt:8.2f} {mt - mp:+14.2f} {spread:14.2f}  {'yes' if inside else 'NO'}")
    return 0 if ok else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--package", default=HERE)
    ap.add_argument("--against", default=None)
    ap.add_argument("--count", action="store_true", help="with --package: function calls per operator call instead of us")
    a = ap.parse_args()
    sys.exit(against(os.path.abspath(a.against)) if a.against else one_run(os.path.abspath(a.package), a.count))
