#!/usr/bin/env python3
"""Fused heat-map peak extraction vs the torch composition it replaces (mmdet's get_local_maximum + get_topk_from_heatmap).

Sizes: the project's headline map 64 x 1 x 1080 x 1920 f32 (531 MB, beyond the 256 MB Infinity Cache, so back-to-back
iterations read from HBM; its share of 8 TB/s by the bytes of the map is reported), CenterPoint / TransFusion
4 x 10 x 180 x 180 f32 with k = 500 and 200 and per class with k = 500 (5.2 MB), CenterNet 32 x 80 x 128 x 128 bf16 with
k = 100 (84 MB).  All but the headline map stay in the Infinity Cache between iterations.  Maps are seeded uniform
noise (about one local maximum in nine elements with kernel 3, a hard case for the selection).  Times are medians of
device-event-timed iterations of accvlab.draw_heatmap.heatmap_peaks and of the composition below.  Prints ONE JSON line.

    python3 scripts/bench_heatmap_peaks.py [--warmup 10] [--iters 50] [--out FILE]
"""
import json
import statistics

import torch
import torch.nn.functional as F

from measure import call_times, emit, gpu, parser

HBM_BPS = 8.0e12
CASES = [
    # name, shape, dtype, k, per_class
    ("headline_64x1x1080x1920_f32_k100", (64, 1, 1080, 1920), torch.float32, 100, False),
    ("centerpoint_4x10x180x180_f32_k500", (4, 10, 180, 180), torch.float32, 500, False),
    ("centerpoint_4x10x180x180_f32_k200", (4, 10, 180, 180), torch.float32, 200, False),
    ("centerpoint_4x10x180x180_f32_k500_per_class", (4, 10, 180, 180), torch.float32, 500, True),
    ("centernet_32x80x128x128_bf16_k100", (32, 80, 128, 128), torch.bfloat16, 100, False),
]


def composition(heat, k, kernel=3, per_class=False):
    """what a head writes today (mmdet models/utils/gaussian_target.py)"""
    B, C, H, W = heat.shape
    hmax = F.max_pool2d(heat, kernel, stride=1, padding=(kernel - 1) // 2)
    heat = heat * (hmax == heat).float()
    scores, inds = torch.topk(heat.view(B * C, -1) if per_class else heat.view(B, -1), k)
    clses, inds = inds // (H * W), inds % (H * W)
    ys, xs = inds // W, inds % W
    return scores, inds, clses, ys, xs


def main():
    args = parser(warmup=10, iters=50).parse_args()

    from accvlab.draw_heatmap import heatmap_peaks

    dev = gpu()
    result = {"metric": "heatmap_peaks_ms", "unit": "ms", "kernel": 3, "warmup": args.warmup, "iters": args.iters,
              "hbm_peak_tbps": 8.0, "cases": {}}
    for name, shape, dtype, k, per_class in CASES:
        g = torch.Generator(device=dev)
        g.manual_seed(42)
        heat = torch.rand(shape, device=dev, generator=g).to(dtype)
        x = heat[:, 0] if shape[1] == 1 else heat    # the headline map is [B, H, W]
        fused = heatmap_peaks(x, k, per_class=per_class)
        comp = composition(heat, k, per_class=per_class)
        # torch.topk orders equal scores arbitrarily: compare the scores, which are equal as multisets in sorted order
        scores_equal = torch.equal(fused.scores.reshape(-1, k).float(), comp[0].reshape(-1, k).float())
        ms_fused, ms_torch = (statistics.median(call_times({"f": f}, args.warmup, args.iters)["f"])     # one after the other
                              for f in (lambda: heatmap_peaks(x, k, per_class=per_class), lambda: composition(heat, k, per_class=per_class)))
        nbytes = heat.numel() * heat.element_size()
        entry = {"shape": list(shape), "dtype": str(dtype).replace("torch.", ""), "k": k, "per_class": per_class,
                 "map_bytes": nbytes, "in_infinity_cache": nbytes < 256 * 2 ** 20, "fused_ms": round(ms_fused, 4),
                 "torch_ms": round(ms_torch, 4), "speedup": round(ms_torch / ms_fused, 2), "scores_equal": scores_equal}
        if not entry["in_infinity_cache"]:
            entry["fused_hbm_fraction"] = round(nbytes / (ms_fused * 1e-3) / HBM_BPS, 3)
        result["cases"][name] = entry
        del heat, x, fused, comp
    result["value"] = result["cases"][CASES[0][0]]["fused_ms"]
    emit([json.dumps(result)], args.out)


if __name__ == "__main__":
    main()
