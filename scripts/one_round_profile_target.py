#!/usr/bin/env python3
"""rocprofv3 target: the densest 8-frame shard (frames 24-31) of the 64-frame headline batch (seed 42, rule A), a one-round
fused-clear launch of 4080 tiles of 128 x 32 pixels, 300 warm-up + 1000 back-to-back launches through the bare C-ABI.  The
library is the shipped one or the build named by ACCV_HIP_LIB (scripts/build_prev_lib.sh for the parent commit):
`rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python scripts/one_round_profile_target.py`"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "accv-lab_amd")]

import torch  # noqa: E402

import bench_workloads as wl  # noqa: E402
from accvlab import _amd_native as nat  # noqa: E402

dev = torch.device("cuda", 0)
B, H, W, lo, frames = 64, 1080, 1920, 24, 8
cl, rl = wl.heatmap_objects(B, H, W, 1, 128, "A", seed=42)
cpad, sizes = wl.pad_ragged(cl)
rpad, _ = wl.pad_ragged(rl)
c, r, n = cpad.to(dev), rpad.to(dev), sizes.to(dev)
nmax = r.shape[1]
hm = torch.empty((B, H, W), device=dev)
lib = nat.lib()
stream = torch.cuda.current_stream().cuda_stream
for _ in range(1300):
    nat.check(lib.accv_draw_heatmap_batched_f32(hm.data_ptr() + lo * H * W * 4, frames, 0, H, W, c.data_ptr() + lo * nmax * 8,
                                                r.data_ptr() + lo * nmax * 4, n.data_ptr() + lo * 8, None, nmax, 6.0, 1.0,
                                                nat.HM_CLEAR | nat.HM_COUNTS_I64, stream), "draw")
torch.cuda.synchronize()
print("ok", nat.LIB_PATH)
