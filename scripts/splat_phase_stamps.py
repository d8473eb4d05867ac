#!/usr/bin/env python3
"""Where does the time of a ONE-ROUND fused-clear splat launch go?  Per-wave phase stamps of the 8-frame shards of the 64-frame
headline batch (seed 42, rule A; 4080 tiles of 128 x 32 pixels, all resident at once), read from a DIAGNOSTIC build of the
library: scripts/build_variant_lib.sh stamps -DACCV_SPLAT_STAMPS [-DACCV_SPLAT_PRIO=0 ...], then
`python scripts/splat_phase_stamps.py accv-lab_amd/accvlab/_amd_native/libaccv_hip_stamps.so [more stamp builds ...]`.

Every tile wave records the 100 MHz constant clock at its start, the time it spent in its cull rounds, row tables and accumulate
loops, the end of its last arithmetic phase and the time after its last store was issued, with its hit count and XCC.  Bare
C-ABI calls, 300 warm-up launches, then back-to-back launches; the records of the last launch of each series are read.  The
stamped build runs longer than the shipped one (its stamps pin the program order): read shares and order, not lengths."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "accv-lab_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench_workloads as wl  # noqa: E402
from accvlab import _amd_native as nat  # noqa: E402

TICK_US = 0.01      # s_memrealtime counts at 100 MHz


def pct(a, q):
    return round(float(np.percentile(a, q)) * TICK_US, 2) if len(a) else None


def main():
    dev = torch.device("cuda", 0)
    B, H, W, frames = 64, 1080, 1920, 8
    cl, rl = wl.heatmap_objects(B, H, W, 1, 128, "A", seed=42)
    cpad, sizes = wl.pad_ragged(cl)
    rpad, _ = wl.pad_ragged(rl)
    c, r, n = cpad.to(dev), rpad.to(dev), sizes.to(dev)
    nmax = r.shape[1]
    hm = torch.empty((B, H, W), device=dev)
    records = frames * ((H + 31) // 32) * ((W + 127) // 128)
    side = torch.zeros((records, 8), dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    flags = nat.HM_CLEAR | nat.HM_COUNTS_I64

    for path in [a for a in sys.argv[1:] if a.endswith(".so")]:
        h = ctypes.CDLL(os.path.abspath(path))
        h.accv_draw_heatmap_batched_f32.restype, h.accv_draw_heatmap_batched_f32.argtypes = nat.SIGNATURES["accv_draw_heatmap_batched_f32"]
        h.accv_debug_splat_stamps.restype, h.accv_debug_splat_stamps.argtypes = None, [ctypes.c_void_p, ctypes.c_longlong]
        h.accv_debug_splat_stamps(side.data_ptr(), records)
        name = os.path.basename(path).replace("libaccv_hip_", "").replace(".so", "")

        def one(k):
            lo = k * frames
            nat.check(h.accv_draw_heatmap_batched_f32(hm.data_ptr() + lo * H * W * 4, frames, 0, H, W, c.data_ptr() + lo * nmax * 8,
                                                      r.data_ptr() + lo * nmax * 4, n.data_ptr() + lo * 8, None, nmax, 6.0, 1.0,
                                                      flags, stream), "draw")

        shards = []
        for k in range(B // frames):
            for _ in range(300):
                one(k)
            series = []
            for _ in range(5):       # five series of 40 back-to-back launches; the last launch of each is read
                side.zero_()
                for _ in range(40):
                    one(k)
                torch.cuda.synchronize()
                series.append(side.cpu().numpy().astype(np.int64))
            shards.append(series)
        hits_of = [int((s[0][:, 7] & 0xffff).sum()) for s in shards]
        for label, k in (("densest", int(np.argmax(hits_of))), ("lightest", int(np.argmin(hits_of)))):
            per_series = []
            for rec in shards[k]:
                t0 = rec[:, 0].min()
                hits = rec[:, 7] & 0xffff
                start, arith_end, done = rec[:, 0] - t0, rec[:, 4] - t0, rec[:, 6] - t0
                order = np.argsort(done)
                tail = order[-41:]          # the last 1 % of the waves to issue their last store
                median_done = float(np.median(done))
                per_series.append({
                    "phase_us_p50_p99_max": {
                        "start_after_first_wave": [pct(start, 50), pct(start, 99), pct(start, 100)],
                        "cull": [pct(rec[:, 1], 50), pct(rec[:, 1], 99), pct(rec[:, 1], 100)],
                        "row_table": [pct(rec[:, 2], 50), pct(rec[:, 2], 99), pct(rec[:, 2], 100)],
                        "accumulate": [pct(rec[:, 3], 50), pct(rec[:, 3], 99), pct(rec[:, 3], 100)],
                        "store_issue": [pct(rec[:, 6] - rec[:, 4], 50), pct(rec[:, 6] - rec[:, 4], 99), pct(rec[:, 6] - rec[:, 4], 100)],
                    },
                    "last_store_issued_us": {"last_wave": pct(done, 100), "p99_wave": pct(done, 99), "median_wave": pct(done, 50)},
                    "arithmetic_ends_us": {"last_wave": pct(arith_end, 100), "p99_wave": pct(arith_end, 99), "median_wave": pct(arith_end, 50)},
                    "last_1pct_waves": {"hits_mean": round(float(hits[tail].mean()), 2), "hits_min": int(hits[tail].min()),
                                        "start_us_mean": round(float(start[tail].mean()) * TICK_US, 2),
                                        "accumulate_us_mean": round(float(rec[tail, 3].mean()) * TICK_US, 2),
                                        "arithmetic_ends_after_median_wave_stored": int((arith_end[tail] > median_done).sum())},
                    "last_wave": {"hits": int(hits[order[-1]]), "start_us": pct(start[order[-1:]], 50),
                                  "arithmetic_ends_us": pct(arith_end[order[-1:]], 50), "xcc": int(rec[order[-1], 7] >> 32)},
                    "heaviest_wave": {"hits": int(hits.max()), "last_store_issued_us": pct(done[np.argmax(hits):np.argmax(hits) + 1], 50),
                                      "accumulate_us": pct(rec[np.argmax(hits):np.argmax(hits) + 1, 3], 50)},
                    "hits_vs_finish_rank_correlation": round(float(np.corrcoef(np.argsort(np.argsort(hits)), np.argsort(order))[0, 1]), 3),
                    "waves_per_xcc": np.bincount((rec[:, 7] >> 32).astype(np.int64), minlength=8).tolist(),
                })
            mid = sorted(per_series, key=lambda s: s["last_store_issued_us"]["last_wave"])[len(per_series) // 2]
            print(json.dumps({"build": name, "shard": label, "frames": [k * frames, (k + 1) * frames], "tiles": records,
                              "hits_total": hits_of[k],
                              "last_store_issued_us_last_wave_all_series": [s["last_store_issued_us"]["last_wave"] for s in per_series],
                              "median_series": mid}), flush=True)
        h.accv_debug_splat_stamps(None, 0)


if __name__ == "__main__":
    main()
