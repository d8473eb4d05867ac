#!/usr/bin/env python3
"""camera_augment_boxes on the GPU against the float64 evaluation of its definition (oracle (b) of tests/camera_boxes_cases.py),
case by case: per output tensor the largest error of an element in units of 2^-24 x the largest magnitude among that
element's float64 intermediates, next to the bar the tests hold it to (the roundings that feed an element).  Every case
also has to equal the float32 oracle exactly, or the script stops.

    python3 scripts/camera_boxes_accuracy.py [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "accv-lab_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the log to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("camera_boxes_accuracy.py measures on a GPU; none is visible")
    import camera_boxes_cases as cases

    lines, worst = [], {}
    for name in sorted(cases.B_CASES):
        case, a = cases.built(name)
        got = cases.run(case, "cuda")
        cases.assert_same(got, a, f"{name}:")
        for tensor, (ratio, n) in cases.check_against_b(got, case, a, report=lines, what=name).items():
            kind = tensor.split("[")[0]
            worst[kind] = max(worst.get(kind, (0.0, n)), (ratio, n))
    lines.append(f"{torch.cuda.get_device_name(0)}: every case equals the float32 oracle on every output tensor; largest error over "
                 f"{len(cases.B_CASES)} cases, in 2^-24 x the element's largest intermediate: "
                 + ", ".join(f"{k} {r:.3f} (bar {n})" for k, (r, n) in sorted(worst.items())))
    print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
