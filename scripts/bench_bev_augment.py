#!/usr/bin/env python3
"""bev_augment_boxes (one launch) vs a vectorised torch composition of its definition, written here.

Two workloads: B = 64 and B = 4 frames, N in [1, 128] objects per frame (ragged, seed 42), D = 9, labels, `valid` true at
0.9, the range check on the raw centres (+-51.2 m, -5 .. 3 m), lidar2img and extrinsics [B, 6, 4, 4] each and ego_to_world
[B, 1, 4, 4] as point transforms, world_to_ego [B, 1, 4, 4] as frame transform.  The composition is what a user gets
without a Python loop over frames: rotate, scale, translate, wrap, compare, one bmm per matrix tensor against A or A^-1
(built on the device from the rows), and one `batched_bool_indexing` per per-object field, whose width is read back from
the device as in the reference.  It is NOT the per-sample numba loop of the reference, which would flatter the operator.

Both alternate inside one process: a timed window is `--calls` back-to-back calls of one side between two device events,
its time divided by the number of calls; `--iters` windows per side; median and minimum per call over the windows.  Launch
counts come from torch's profiler in a separate pass (kernel events per call; copies and memsets are not counted); "not
measured" if the profiler is unavailable.  Host round trips are the synchronising calls torch's sync debug mode reports in
one call.  The fused outputs are compared per tensor with the composition evaluated on float64 copies of the inputs,
within the bar of the tests, n * 2^-24 * the tensor's largest magnitude (n = 5 boxes, 9 point transforms, 5 frame
transforms; a yaw may differ by a whole turn; integer outputs must be equal).  Prints a few lines of log per workload and
ONE JSON line.

    python3 scripts/bench_bev_augment.py [--warmup 20] [--iters 200] [--calls 50] [--out FILE]
"""
import json
import math

import torch

from measure import emit, gpu, launches, parser, round_trips, shown, summary, window_times

RANGE = ((-51.2, -51.2, -5.0), (51.2, 51.2, 3.0))
BARS = dict(boxes=5, point=9, frame=5)


def poses(g, B, K, spread):
    q, _ = torch.linalg.qr(torch.randn(B, K, 3, 3, generator=g, dtype=torch.float64))
    m = torch.zeros(B, K, 4, 4, dtype=torch.float64)
    m[..., :3, :3] = q
    m[..., :3, 3] = (torch.rand(B, K, 3, generator=g, dtype=torch.float64) * 2 - 1) * spread
    m[..., 3, 3] = 1.0
    return m


def make_inputs(B, n_max, dev, seed=42):
    from accvlab.draw_heatmap import bev_augmentation_params

    g = torch.Generator().manual_seed(seed)
    sizes = torch.randint(1, n_max + 1, (B,), generator=g)
    N = int(sizes.max())
    u = lambda *s: torch.rand(*s, generator=g)   # noqa: E731
    boxes = torch.cat([(u(B, N, 2) * 2 - 1) * 70.0, u(B, N, 1) * 10 - 6, 0.3 + u(B, N, 3) * 11.7, (u(B, N, 1) * 2 - 1) * math.pi,
                       u(B, N, 2) * 20 - 10], -1).to(torch.float32).contiguous()
    labels = torch.randint(0, 10, (B, N), generator=g)
    valid = u(B, N) < 0.9
    rows = bev_augmentation_params((u(B) * 2 - 1) * 0.3925, 0.95 + u(B) * 0.1, (u(B, 3) * 2 - 1) * 0.5)
    ego = poses(g, B, 1, 2000.0)
    cams = poses(g, B, 6, 3.0)
    intr = torch.tensor([[1260.0, 0, 800, 0], [0, 1260.0, 450, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=torch.float64)
    mats = dict(lidar2img=(intr @ cams).float(), extrinsics=cams.float(), ego_to_world=ego.float(), world_to_ego=torch.linalg.inv(ego).float())
    return (boxes.to(dev), labels.to(dev), valid.to(dev), sizes.to(dev), rows.to(dev), {k: v.contiguous().to(dev) for k, v in mats.items()})


def constants(dev):
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)   # noqa: E731
    return dict(lo=f32(RANGE[0]), hi=f32(RANGE[1]), pi=f32(math.pi), two_pi=f32(2 * math.pi))


def composition(boxes, labels, valid, sizes, rows, mats, k):
    """the definition over whole tensors, then one batched_bool_indexing per field (each reads its width back)"""
    from accvlab.batching_helpers import RaggedBatch, batched_bool_indexing

    B, N, D = boxes.shape
    th, c, s, sc = (rows[:, i, None] for i in range(4))
    t = rows[:, None, 4:7]
    x, y, z = boxes[..., 0], boxes[..., 1], boxes[..., 2]
    centre = torch.stack([(c * x - s * y) * sc, (s * x + c * y) * sc, z * sc], -1) + t
    v = boxes[..., 6] + th
    v = torch.where(v < -k["pi"], v + torch.ceil((-k["pi"] - v) / k["two_pi"]) * k["two_pi"],
                    torch.where(v > k["pi"], v - torch.ceil((v - k["pi"]) / k["two_pi"]) * k["two_pi"], v))
    vx, vy = boxes[..., 7], boxes[..., 8]
    out = torch.cat([centre, boxes[..., 3:6] * sc[..., None], v[..., None], ((c * vx - s * vy) * sc)[..., None],
                     ((s * vx + c * vy) * sc)[..., None]], -1)
    xyz = boxes[..., :3]
    slot = torch.arange(N, device=boxes.device)
    keep = valid & (xyz >= k["lo"]).all(-1) & (xyz <= k["hi"]).all(-1) & (slot[None] < sizes[:, None])
    zero, one = torch.zeros_like(c), torch.ones_like(c)
    R = torch.stack([torch.cat([c, -s, zero, zero], 1), torch.cat([s, c, zero, zero], 1), torch.cat([zero, zero, one, zero], 1),
                     torch.cat([zero, zero, zero, one], 1)], 1)
    A = R * torch.cat([sc, sc, sc, one], 1)[:, :, None]
    A = torch.cat([A[:, :, :3], torch.cat([t[:, 0], one], 1)[:, :, None]], 2)
    inv3 = R[:, :3, :3].transpose(1, 2) / sc[:, :, None]                       # A^-1 = R^T S^-1 T^-1, in closed form
    Ainv = torch.cat([torch.cat([inv3, -(inv3 @ t.transpose(1, 2))], 2), torch.cat([zero, zero, zero, one], 1)[:, None]], 1)
    pts = tuple(m @ Ainv[:, None] for m in (mats["lidar2img"], mats["extrinsics"], mats["ego_to_world"]))
    frs = (A[:, None] @ mats["world_to_ego"],)
    rb = lambda x: RaggedBatch(x, sample_sizes=sizes)   # noqa: E731
    return (batched_bool_indexing(rb(out), keep), batched_bool_indexing(rb(labels), keep),
            batched_bool_indexing(rb(slot[None].expand(B, N).to(torch.int32).contiguous()), keep), keep, pts, frs)


def differing(got, ref, inputs):
    """the output tensors of the fused call that differ from the composition beyond the bar (integers: at all).  `ref` is
    the composition evaluated on float64 copies of the inputs, so that the bar measures the fused call alone; a tensor's
    magnitude is the largest among its inputs and outputs."""
    u = 2.0 ** -24
    bad = []
    top = lambda x: float(x.abs().max()) if x.numel() else 0.0   # noqa: E731

    def close(name, a, b, n, source):
        a, b = a.double(), b.double()
        mag = max(top(a), top(b), top(source))
        diff = (a - b).abs()
        if name == "boxes":
            diff[..., 6] = torch.minimum(diff[..., 6], (diff[..., 6] - 2 * math.pi).abs())
        if diff.numel() and float(diff.max()) > n * u * mag:
            bad.append(name)

    w = ref[0].tensor.shape[1]
    if not torch.equal(got.boxes.sample_sizes, ref[0].sample_sizes):
        bad.append("sizes")
    boxes, p_in, f_in = inputs
    close("boxes", got.boxes.tensor[:, :w], ref[0].tensor, BARS["boxes"], boxes)
    if not torch.equal(got.labels.tensor[:, :w], ref[1].tensor):
        bad.append("labels")
    if not torch.equal(got.source.tensor[:, :w].clamp(min=0), ref[2].tensor):      # the composition pads with 0
        bad.append("source")
    if not torch.equal(got.keep.tensor, ref[3]):
        bad.append("keep")
    for i, (a, b) in enumerate(zip(got.point_transforms, ref[4])):
        close(f"point_transforms[{i}]", a, b, BARS["point"], p_in[i])
    for i, (a, b) in enumerate(zip(got.frame_transforms, ref[5])):
        close(f"frame_transforms[{i}]", a, b, BARS["frame"], f_in[i])
    return bad


def workload(B, args, dev):
    from accvlab.batching_helpers import RaggedBatch
    from accvlab.draw_heatmap import bev_augment_boxes

    boxes, labels, valid, sizes, rows, mats = make_inputs(B, args.n_max, dev)
    rb, rl = RaggedBatch(boxes, sample_sizes=sizes), RaggedBatch(labels, sample_sizes=sizes)
    k = constants(dev)
    p_in = (mats["lidar2img"], mats["extrinsics"], mats["ego_to_world"])
    fused = lambda: bev_augment_boxes(rb, rows, labels=rl, valid=valid, point_range=RANGE, point_transforms=p_in,       # noqa: E731
                                      frame_transforms=(mats["world_to_ego"],))
    comp = lambda: composition(boxes, labels, valid, sizes, rows, mats, k)                                             # noqa: E731
    got = fused()
    ref = composition(boxes.double(), labels, valid, sizes, rows.double(), {n: m.double() for n, m in mats.items()}, k)
    torch.cuda.synchronize()
    bad = differing(got, ref, (boxes, p_in, (mats["world_to_ego"],)))
    ms = {k: summary(v, args.calls) for k, v in window_times({"fused": fused, "torch": comp}, args.warmup, args.iters, args.calls).items()}
    n = {"fused": launches(fused), "torch": launches(comp)}
    trips = {"fused": shown(round_trips(fused)), "torch": shown(round_trips(comp))}
    result = dict(shape=dict(B=B, N=int(boxes.shape[1]), D=9, point_transforms=[list(m.shape) for m in p_in],
                             frame_transforms=[list(mats["world_to_ego"].shape)]),
                  objects=int(sizes.sum()), kept=int(got.boxes.sample_sizes.sum()), fused=ms["fused"], torch=ms["torch"],
                  speedup_median=round(ms["torch"]["median_ms"] / ms["fused"]["median_ms"], 2),
                  launches_fused=shown(n["fused"]), launches_torch=shown(n["torch"]), host_round_trips_fused=trips["fused"],
                  host_round_trips_torch=trips["torch"], tensors_beyond_the_bar=bad)
    lines = [f"bev_augment_boxes  B={B} N<={boxes.shape[1]} D=9, 3 point transforms (6 + 6 + 1 matrices per frame), 1 frame transform: "
             f"{int(sizes.sum())} objects, {result['kept']} kept",
             f"  {args.iters} windows of {args.calls} calls per side, alternating; timed {ms['fused']['timed_s']} s fused, {ms['torch']['timed_s']} s torch",
             f"  fused   median {ms['fused']['median_ms']:.4f} ms  min {ms['fused']['min_ms']:.4f} ms  launches {result['launches_fused']}  "
             f"host round trips {trips['fused']}",
             f"  torch   median {ms['torch']['median_ms']:.4f} ms  min {ms['torch']['min_ms']:.4f} ms  launches {result['launches_torch']}  "
             f"host round trips {trips['torch']}",
             f"  output tensors that differ from the torch composition beyond the bar: {len(bad)} {bad}"]
    return result, lines


def main():
    ap = parser(warmup=20, iters=200, calls=50)
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 4])
    ap.add_argument("--n-max", type=int, default=128)
    args = ap.parse_args()
    dev = gpu()
    results, lines = [], []
    for B in args.batches:
        r, ls = workload(B, args, dev)
        results.append(r)
        lines += ls
    first = results[0]
    lines.append(json.dumps(dict(metric="bev_augment_boxes_ms", unit="ms", value=first["fused"]["median_ms"], warmup=args.warmup,
                                 iters=args.iters, calls_per_window=args.calls, workloads=results)))
    emit(lines, args.out)


if __name__ == "__main__":
    main()
