#!/usr/bin/env python3
"""camera_augment_boxes (one launch) vs a composition of what the package offered before it, written here.

Two workloads (ragged, seed 42): 48 frames of up to 64 boxes and 64 frames of up to 128 boxes, 900 x 1600 annotations
brought to 256 x 704 by flip + scale + crop matrices (sample_image_transforms with the StreamPETR recipe, one draw per
group of 6 cameras), the occlusion check and minimum_size = 2, categories (a tenth negative), centres, lidar2img as
[F, 4, 4] and intrinsics as [F, 3, 3].  The composition: the point warp as elementwise torch operations in the order of
the definition (so that its decisions are the operator's), one matmul per matrix tensor, `visible_bbox_mask` on the warped
boxes, the condition, one `batched_bool_indexing` per field (each reads its width back from the device), `clamp`.

Both alternate inside one process: a timed window is `--calls` back-to-back calls of one side between two device events,
its time divided by the number of calls; `--iters` windows per side; median and minimum per call over the windows.  Launch
counts come from torch's profiler in a separate pass (kernel events per call; copies and memsets are not counted); "not
measured" if the profiler is unavailable.  Host round trips are the synchronising calls torch's sync debug mode reports in
one call.  The fused outputs are compared per tensor with the composition: flags, sources, categories and counts must be
equal, coordinates lie within 4 * 2^-24 * the tensor's largest magnitude, and the matrices within 5 * 2^-24 * the largest
magnitude of the composition evaluated on float64 copies (the bars of the tests).  Prints a few lines of log per workload
and ONE JSON line.

`--entry-only` times the C entry alone instead, on outputs allocated once: the launch and the kernel without the Python of
the operator around them.

    python3 scripts/bench_camera_boxes.py [--warmup 20] [--iters 200] [--calls 50] [--entry-only] [--out FILE]
"""
import json

import torch

from measure import emit, gpu, launches, parser, round_trips, shown, summary, timed_windows, window_times

WORKLOADS = ((48, 64), (64, 128))
SOURCE_HW, OUTPUT_HW = (900, 1600), (256, 704)
MIN_SIZE = 2.0
BARS = dict(point=4, matrix=5)


def make_inputs(Fr, n_max, dev, seed=42):
    from accvlab.image_prep import (NonUniformScaling, ShiftToAlignWithOriginalImageBorder, UniformScaling,
                                    sample_image_transforms)

    g = torch.Generator().manual_seed(seed)
    sizes = torch.randint(1, n_max + 1, (Fr,), generator=g)
    G = int(sizes.max())
    H, W = SOURCE_HW
    u = lambda *s: torch.rand(*s, generator=g)   # noqa: E731
    cx, cy = (u(Fr, G) * 1.2 - 0.1) * W, (u(Fr, G) * 1.2 - 0.1) * H
    w, h = 4 + u(Fr, G) ** 3 * W / 3, 4 + u(Fr, G) ** 3 * H / 3
    boxes = torch.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], -1).to(torch.float32).contiguous()
    centers = torch.stack([cx, cy], -1).to(torch.float32).contiguous()
    depths = (1 + u(Fr, G) * 79).to(torch.float32)
    cats = torch.randint(0, 10, (Fr, G), generator=g)
    cats[u(Fr, G) < 0.1] = -1
    steps = [NonUniformScaling(0.5, (-1.0, 1.0)), UniformScaling(1.0, 0.9, 1.1), ShiftToAlignWithOriginalImageBorder(1.0, "bottom")]
    t = sample_image_transforms(Fr // 6 + 1, 6, steps, source_hw=SOURCE_HW, output_hw=OUTPUT_HW, mode="crop", anchor="bottom_or_right",
                                generator=g)[:Fr].contiguous()
    intr = torch.tensor([[1260.0, 0, 800], [0, 1260.0, 450], [0, 0, 1]], dtype=torch.float64).expand(Fr, 3, 3)
    q, _ = torch.linalg.qr(torch.randn(Fr, 3, 3, generator=g, dtype=torch.float64))
    ext = torch.zeros(Fr, 4, 4, dtype=torch.float64)
    ext[:, :3, :3], ext[:, :3, 3], ext[:, 3, 3] = q, (u(Fr, 3).double() * 2 - 1) * 3.0, 1.0
    k4 = torch.zeros(Fr, 4, 4, dtype=torch.float64)
    k4[:, :3, :3], k4[:, 3, 3] = intr, 1.0
    mats = ((k4 @ ext).float().contiguous(), intr.float().contiguous())
    return tuple(x.to(dev) for x in (boxes, centers, depths, cats, sizes, t)) + (tuple(m.to(dev) for m in mats),)


def composition(boxes, centers, depths, cats, sizes, t, mats, hw):
    from accvlab.batching_helpers import RaggedBatch
    from accvlab.draw_heatmap import visible_bbox_mask

    a, b, tx, c, d, ty = (t[:, i, j, None] for i in range(2) for j in range(3))
    warp = lambda x, y: ((a * x + b * y) + tx, (c * x + d * y) + ty)   # noqa: E731
    x1, y1 = warp(boxes[..., 0], boxes[..., 1])
    x2, y2 = warp(boxes[..., 2], boxes[..., 3])
    wb = torch.stack([x1, y1, x2, y2], -1)
    wc = torch.stack(warp(centers[..., 0], centers[..., 1]), -1)
    A3 = torch.cat([t, torch.tensor([[[0.0, 0.0, 1.0]]], dtype=t.dtype, device=t.device).expand(t.shape[0], 1, 3)], 1)
    new_mats = []
    for m in mats:
        top = A3 @ m[:, :3]
        new_mats.append(torch.cat([top[:, :2], m[:, 2:]], 1))
    rb = lambda x: RaggedBatch(x, sample_sizes=sizes)   # noqa: E731
    if wb.dtype == torch.float32:
        visible = visible_bbox_mask(rb(wb.contiguous()), depths, image_hw=hw, minimum_size=MIN_SIZE).tensor
    else:
        visible = None
    return wb, wc, visible, new_mats, rb


def compact(wb, wc, visible, depths, cats, sizes, rb, hw):
    from accvlab.batching_helpers import batched_bool_indexing

    keep = visible & (cats >= 0)
    H, W = hw
    lim = torch.tensor([W, H, W, H], dtype=wb.dtype, device=wb.device)
    ob = batched_bool_indexing(rb(wb), keep)
    oc = batched_bool_indexing(rb(wc), keep)
    od = batched_bool_indexing(rb(depths), keep)
    ok = batched_bool_indexing(rb(cats), keep)
    zero = torch.zeros((), dtype=wb.dtype, device=wb.device)
    return (ob.tensor.clamp(zero, lim), oc.tensor.clamp(zero, lim[:2]), od.tensor, ok.tensor, ob.sample_sizes, keep, visible)


def baseline(boxes, centers, depths, cats, sizes, t, mats, hw):
    wb, wc, visible, new_mats, rb = composition(boxes, centers, depths, cats, sizes, t, mats, hw)
    return compact(wb, wc, visible, depths, cats, sizes, rb, hw) + (new_mats,)


def differing(got, ref, ref_mats64, inputs):
    """the output tensors of the fused call that differ from the composition beyond the bars"""
    u = 2.0 ** -24
    bad = []
    top = lambda x: float(x.abs().max()) if x.numel() else 0.0   # noqa: E731
    ob, oc, od, ok, kept, keep, visible, _ = ref
    w = ob.shape[1]
    if not torch.equal(got.bboxes.sample_sizes, kept.to(torch.int64)):
        bad.append("sizes")
    for name, a, b, src in (("bboxes", got.bboxes.tensor[:, :w], ob, inputs[0]), ("centers", got.centers.tensor[:, :w], oc, inputs[1])):
        if a.numel() and float((a.double() - b.double()).abs().max()) > BARS["point"] * u * max(top(a), top(b), top(src)):
            bad.append(name)
    if not torch.equal(got.depths.tensor[:, :w], od):
        bad.append("depths")
    if not torch.equal(got.categories.tensor[:, :w], ok):
        bad.append("categories")
    if not torch.equal(got.keep.tensor, keep):
        bad.append("keep")
    if not torch.equal(got.visible.tensor, visible):
        bad.append("visible")
    if bool(got.bboxes.tensor[:, w:].any()) or bool((got.source.tensor[:, w:] != -1).any()):
        bad.append("padding")
    t64 = inputs[3].double()
    for i, (a, b, src) in enumerate(zip(got.projection_matrices, ref_mats64, inputs[2])):
        products = t64[:, :, :, None] * src.double()[:, None, :3, :]          # every a*m0j, b*m1j, tx*m2j
        if float((a.double() - b).abs().max()) > BARS["matrix"] * u * max(top(products), top(b), top(src)):
            bad.append(f"projection_matrices[{i}]")
    return bad


def workload(Fr, n_max, args, dev):
    from accvlab.batching_helpers import RaggedBatch
    from accvlab.draw_heatmap import camera_augment_boxes
    from accvlab.image_prep import padded_hw

    boxes, centers, depths, cats, sizes, t, mats = make_inputs(Fr, n_max, dev)
    hw = padded_hw(OUTPUT_HW, 32)
    rb = RaggedBatch(boxes, sample_sizes=sizes)
    fused = lambda: camera_augment_boxes(rb, t, image_hw=hw, centers=centers, depths=depths, categories=cats,     # noqa: E731
                                         minimum_size=MIN_SIZE, projection_matrices=mats)
    comp = lambda: baseline(boxes, centers, depths, cats, sizes, t, mats, hw)                                      # noqa: E731
    got, ref = fused(), comp()
    mats64 = composition(boxes.double(), centers.double(), depths, cats, sizes, t.double(), tuple(m.double() for m in mats), hw)[3]
    torch.cuda.synchronize()
    bad = differing(got, ref, mats64, (boxes, centers, mats, t))
    ms = {k: summary(v, args.calls) for k, v in window_times({"fused": fused, "torch": comp}, args.warmup, args.iters, args.calls).items()}
    n = {"fused": launches(fused), "torch": launches(comp)}
    trips = {"fused": shown(round_trips(fused)), "torch": shown(round_trips(comp))}
    result = dict(shape=dict(F=Fr, G=int(boxes.shape[1]), image_hw=list(hw), projection_matrices=[list(m.shape) for m in mats]),
                  boxes=int(sizes.sum()), visible=int(got.visible.tensor.sum()), kept=int(got.bboxes.sample_sizes.sum()),
                  fused=ms["fused"], torch=ms["torch"], speedup_median=round(ms["torch"]["median_ms"] / ms["fused"]["median_ms"], 2),
                  launches_fused=shown(n["fused"]), launches_torch=shown(n["torch"]), host_round_trips_fused=trips["fused"],
                  host_round_trips_torch=trips["torch"], tensors_beyond_the_bar=bad)
    lines = [f"camera_augment_boxes  F={Fr} frames, G<={boxes.shape[1]}, {SOURCE_HW[0]}x{SOURCE_HW[1]} -> {hw[0]}x{hw[1]}, occlusion + "
             f"minimum_size {MIN_SIZE:g}, categories, centres, lidar2img [F, 4, 4], intrinsics [F, 3, 3]: {int(sizes.sum())} boxes, "
             f"{result['visible']} visible, {result['kept']} kept",
             f"  {args.iters} windows of {args.calls} calls per side, alternating; timed {ms['fused']['timed_s']} s fused, {ms['torch']['timed_s']} s torch",
             f"  fused   median {ms['fused']['median_ms']:.4f} ms  min {ms['fused']['min_ms']:.4f} ms  launches {result['launches_fused']}  "
             f"host round trips {trips['fused']}",
             f"  torch   median {ms['torch']['median_ms']:.4f} ms  min {ms['torch']['min_ms']:.4f} ms  launches {result['launches_torch']}  "
             f"host round trips {trips['torch']}",
             f"  output tensors that differ from the torch composition beyond the bars: {len(bad)} {bad}"]
    return result, lines


def entry_alone(Fr, n_max, args, dev):
    """the C entry alone on outputs allocated once: the launch and the kernel without the Python of the operator"""
    import ctypes

    from accvlab import _amd_native as nat
    from accvlab.batching_helpers import RaggedBatch
    from accvlab.draw_heatmap import camera_augment_boxes
    from accvlab.image_prep import padded_hw

    boxes, centers, depths, cats, sizes, t, mats = make_inputs(Fr, n_max, dev)
    hw = padded_hw(OUTPUT_HW, 32)
    out = camera_augment_boxes(RaggedBatch(boxes, sample_sizes=sizes), t, image_hw=hw, centers=centers, depths=depths, categories=cats,
                               minimum_size=MIN_SIZE, projection_matrices=mats)       # its tensors serve as the outputs
    prm = nat.CameraBoxesParams()
    prm.minimum_size, prm.image_h, prm.image_w = MIN_SIZE, hw[0], hw[1]
    for i, (src, dst) in enumerate(zip(mats, out.projection_matrices)):
        prm.mat_in[i], prm.mat_out[i], prm.mat_count[i] = src.data_ptr(), dst.data_ptr(), 1
        prm.mat_rows[i], prm.mat_cols[i] = src.shape[-2], src.shape[-1]
    prm.num_matrices, prm.check_occlusion, prm.check_size, prm.crop = len(mats), 1, 1, 1
    cargs = (boxes.data_ptr(), t.data_ptr(), centers.data_ptr(), depths.data_ptr(), cats.data_ptr(), None, sizes.data_ptr(),
             nat.CB_COUNTS_I64 | nat.CB_CATEGORIES_I64, Fr, int(boxes.shape[1]), ctypes.addressof(prm), out.bboxes.tensor.data_ptr(),
             out.centers.tensor.data_ptr(), out.depths.tensor.data_ptr(), out.categories.tensor.data_ptr(), out.source.tensor.data_ptr(),
             out.keep.tensor.data_ptr(), out.visible.tensor.data_ptr(), out.bboxes.sample_sizes.data_ptr(), nat.stream_ptr(dev))
    entry = nat.lib().accv_camera_boxes
    want = [x.clone() for x in (out.bboxes.tensor, out.keep.tensor, out.bboxes.sample_sizes)]

    def call():
        assert entry(*cargs) == 0

    ms = timed_windows(call, args.warmup, args.iters, args.calls)
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) for a, b in zip(want, (out.bboxes.tensor, out.keep.tensor, out.bboxes.sample_sizes)))
    line = (f"accv_camera_boxes alone  F={Fr} frames, G<={boxes.shape[1]}: {args.iters} windows of {args.calls} calls; "
            f"median {ms['median_ms']:.4f} ms  min {ms['min_ms']:.4f} ms  outputs equal to the operator's: {same}")
    return dict(F=Fr, G=int(boxes.shape[1]), entry=ms, outputs_equal=same), [line]


def main():
    ap = parser(warmup=20, iters=200, calls=50)
    ap.add_argument("--entry-only", action="store_true", help="time the C entry alone on outputs allocated once, nothing else")
    args = ap.parse_args()
    dev = gpu()
    results, lines = [], []
    if args.entry_only:
        for Fr, n_max in WORKLOADS:
            r, ls = entry_alone(Fr, n_max, args, dev)
            results.append(r)
            lines += ls
        lines.append(json.dumps(dict(metric="accv_camera_boxes_entry_ms", unit="ms", value=results[0]["entry"]["median_ms"],
                                     warmup=args.warmup, iters=args.iters, calls_per_window=args.calls, workloads=results)))
        emit(lines, args.out)
        return
    for Fr, n_max in WORKLOADS:
        r, ls = workload(Fr, n_max, args, dev)
        results.append(r)
        lines += ls
    lines.append(json.dumps(dict(metric="camera_augment_boxes_ms", unit="ms", value=results[0]["fused"]["median_ms"], warmup=args.warmup,
                                 iters=args.iters, calls_per_window=args.calls, workloads=results)))
    emit(lines, args.out)
    if any(r["tensors_beyond_the_bar"] for r in results):
        raise SystemExit("the fused call differs from the composition")


if __name__ == "__main__":
    main()
