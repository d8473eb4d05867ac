#!/usr/bin/env python3
"""rotated_nms_bev (one launch for every task, no host round trip) vs what a user does today for the `rotate` branch of
CenterHead.get_bboxes on this platform: copy the decode's outputs to the host, run a rotated NMS per frame and task there,
copy the kept detections back.

Size: B = 4 frames, the six nuScenes tasks over ten classes, 180 x 180 maps (pc_range +-54 m, voxel 0.075 m, stride 8),
N = K = 500 decoded slots per task and frame (score threshold 0.1, post_center_range +-61.2 m, no NMS in the decode), IoU
threshold 0.2, post_max_size 83; float32 logits and heads, seed 42: the inputs of scripts/bench_center_decode.py.

Three sides alternate inside one process:
  nms alone    rotated_nms_bev on the decode's output (computed once)
  fused        heatmap_peaks + center_point_decode(nms_threshold=None) + rotated_nms_bev from the logits
  round trip   the same NMS on the host: D2H of the decode's four outputs and sizes, the library's OWN host entry (the same
               arithmetic, serial), H2D of the result.  The host NMS is the library's so that the comparison isolates the
               round trips and the serial walk; the decode's output is computed once, as for `nms alone`.
A timed block is `--calls` back-to-back calls of one side between two device events (the round trip synchronises inside;
the events still enclose all of its work), its time divided by the number of calls; `--iters` blocks per side; median and
minimum per call over the blocks, for `nms alone` the maximum too (max - min is the spread a change is held against: run
the script once per library, `ACCV_HIP_LIB` selecting the other build, in turn).  Launch counts come from torch's profiler in a separate pass (kernel events per call;
copies and memsets are not counted); "not measured" if the profiler is unavailable.  Prints a few lines of log and ONE JSON
line.

    python3 scripts/bench_rotated_nms.py [--warmup 20] [--iters 10] [--calls 20] [--out profiles/rotated_nms_bench.log]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))      # the workload below is a sibling's
import torch  # noqa: E402

from bench_center_decode import CFG, OPTS, TASKS, make_inputs  # noqa: E402
from measure import emit, gpu, launches, parser, shown, summary, window_times  # noqa: E402

IOU_THRESHOLD = 0.2
POST_MAX_SIZE = 83


def main():
    ap = parser(warmup=20, iters=10, calls=20)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--k", type=int, default=500)
    args = ap.parse_args()
    dev = gpu()
    from accvlab.batching_helpers import RaggedBatch
    from accvlab.draw_heatmap import CenterPointDetections, center_point_decode, heatmap_peaks, rotated_nms_bev

    logits, heads = make_inputs(args.batch, dev)
    K = args.k
    opts = dict(OPTS, nms_threshold=None, post_max_size=None)

    def decode():
        return center_point_decode([heatmap_peaks(lg, K, kernel=1) for lg in logits], heads, TASKS, **CFG, scores_are_logits=True, **opts)

    dets = decode()

    def nms_only():
        return rotated_nms_bev(dets, IOU_THRESHOLD, post_max_size=POST_MAX_SIZE)

    def fused():
        return rotated_nms_bev(decode(), IOU_THRESHOLD, post_max_size=POST_MAX_SIZE)

    def round_trip():
        host = []
        for d in dets:                                     # D2H: five copies per task, each one synchronises
            sizes = d.boxes.sample_sizes.cpu()
            host.append(CenterPointDetections(*(RaggedBatch(x.tensor.cpu(), sample_sizes=sizes) for x in d)))
        kept = rotated_nms_bev(host, IOU_THRESHOLD, post_max_size=POST_MAX_SIZE)
        out = []
        for d in kept:                                     # H2D
            sizes = d.boxes.sample_sizes.to(dev)
            out.append(CenterPointDetections(*(RaggedBatch(x.tensor.to(dev), sample_sizes=sizes) for x in d)))
        return out

    got, ref = nms_only(), round_trip()
    torch.cuda.synchronize()
    decoded = sum(int(d.boxes.sample_sizes.sum()) for d in dets)
    kept = sum(int(d.boxes.sample_sizes.sum()) for d in got)
    mismatch = 0
    for d, r in zip(got, ref):
        mismatch += int(not torch.equal(d.boxes.sample_sizes, r.boxes.sample_sizes))
        mismatch += sum(int(not torch.equal(x.tensor.view(torch.uint8), y.tensor.view(torch.uint8))) for x, y in zip(d, r))
    ms = window_times({"nms": nms_only, "fused": fused, "round_trip": round_trip}, args.warmup, args.iters, args.calls)
    ms = {k: summary(v, args.calls, with_max=True) for k, v in ms.items()}
    n_nms, n_fused, n_trip = launches(nms_only), launches(fused), launches(round_trip)
    T = len(TASKS)
    result = dict(metric="rotated_nms_bev_ms", unit="ms", value=ms["nms"]["median_ms"], warmup=args.warmup, iters=args.iters,
                  calls_per_block=args.calls, shape=dict(B=args.batch, T=T, N=K, iou_threshold=IOU_THRESHOLD, post_max_size=POST_MAX_SIZE),
                  decoded=decoded, kept=kept, nms=ms["nms"], fused=ms["fused"], round_trip=ms["round_trip"],
                  speedup_median_nms_vs_round_trip=round(ms["round_trip"]["median_ms"] / ms["nms"]["median_ms"], 2),
                  launches_nms=shown(n_nms), launches_fused=shown(n_fused), launches_round_trip=shown(n_trip),
                  host_round_trips=T, host_copies_round_trip=10 * T, tensors_that_differ_from_the_round_trip=mismatch)
    lines = [f"rotated_nms_bev  B={args.batch} T={T} N={K} iou_threshold={IOU_THRESHOLD} post_max_size={POST_MAX_SIZE}: {decoded} decoded, {kept} kept"
             f" on {torch.cuda.get_device_name(0)}",
             f"  {args.warmup} warm-up calls, {args.iters} blocks of {args.calls} calls per side, alternating",
             f"  nms alone           median {ms['nms']['median_ms']:.4f} ms  min {ms['nms']['min_ms']:.4f} ms  max {ms['nms']['max_ms']:.4f} ms  launches {shown(n_nms)}  host round trips 0",
             f"  peaks+decode+nms    median {ms['fused']['median_ms']:.4f} ms  min {ms['fused']['min_ms']:.4f} ms  launches {shown(n_fused)}  host round trips 0",
             f"  D2H, host nms, H2D  median {ms['round_trip']['median_ms']:.4f} ms  min {ms['round_trip']['min_ms']:.4f} ms  launches {shown(n_trip)}  "
             f"host round trips {T} (one per task: 5 copies down, each waiting for the device, and 5 up)",
             f"  against the round trip: {mismatch} output tensors differ",
             json.dumps(result)]
    emit(lines, args.out)


if __name__ == "__main__":
    main()
