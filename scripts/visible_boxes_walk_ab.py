#!/usr/bin/env python3
"""A/B of visible_boxes_kernel across a change of its source: an earlier commit's library (libaccv_hip_prev.so, built by
scripts/build_prev_lib.sh) against the working tree's, in one process, through the C entry alone, on the inputs of
scripts/bench_visible_bboxes.py.  Rounds alternate; the medians of the earlier library's rounds give the run-to-run spread
the working tree's median is held against.  The masks must be equal.

    bash scripts/build_prev_lib.sh HEAD && python3 scripts/visible_boxes_walk_ab.py [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "accv-lab_amd"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import bench_visible_bboxes as bv  # noqa: E402
from accvlab import _amd_native as nat  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the log to this file")
args = ap.parse_args()
ROUNDS, WINDOWS, CALLS = 5, 60, 20
native = os.path.join(ROOT, "accv-lab_amd", "accvlab", "_amd_native")
libs = {"parent": ctypes.CDLL(os.path.join(native, "libaccv_hip_prev.so")), "this": ctypes.CDLL(os.path.join(native, "libaccv_hip.so"))}
for lib in libs.values():
    lib.accv_visible_boxes.restype, lib.accv_visible_boxes.argtypes = nat.SIGNATURES["accv_visible_boxes"]
dev = torch.device("cuda", 0)
stream = nat.stream_ptr(dev)
lines = []
for B, H, W, n_max in bv.SIZES:
    boxes, depths, sizes = bv.make_inputs(B, H, W, n_max, dev)
    hw = torch.tensor([[H, W]] * B, dtype=torch.int32, device=dev)
    prm = nat.VisibleBoxesParams(bv.MIN_SIZE, 0, 0, 1, 1, 0)
    outs = {k: torch.empty(depths.shape, dtype=torch.bool, device=dev) for k in libs}
    G = boxes.shape[1]

    def call(k):
        rc = libs[k].accv_visible_boxes(boxes.data_ptr(), depths.data_ptr(), sizes.data_ptr(), hw.data_ptr(), nat.VB_COUNTS_I64, B, G,
                                        ctypes.addressof(prm), outs[k].data_ptr(), stream)
        assert rc == 0

    for k in libs:
        call(k)
    torch.cuda.synchronize()
    assert torch.equal(outs["parent"], outs["this"]), "the masks differ"
    med = {k: [] for k in libs}
    for r in range(ROUNDS):
        for k in (("parent", "this") if r % 2 == 0 else ("this", "parent")):
            med[k].append(bv.timed_windows(lambda: call(k), 20, WINDOWS, CALLS)["median_ms"])
    for k in libs:
        lines.append(f"visible_boxes_kernel B={B} N<={G} {k:6s}: medians of {ROUNDS} rounds ({WINDOWS} windows of {CALLS} calls) "
                     f"{' '.join(f'{m:.5f}' for m in med[k])} ms; median {statistics.median(med[k]):.5f}  min {min(med[k]):.5f}  max {max(med[k]):.5f}")
    lines.append(json.dumps(dict(B=B, G=G, parent=med["parent"], this=med["this"], masks_equal=True)))
print("\n".join(lines), flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
