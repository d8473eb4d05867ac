#!/usr/bin/env python3
"""The largest error of prepare_images on the GPU against the float64 oracle of tests/image_prep_cases.py, per group of
cases, next to the derived bar (K * 2^-24 * (1 + max saturation) * 255 / min(std), K = 23), and whether the device result
equals the host entry bit for bit.  Prints one line per group and one for the whole set.

    python3 scripts/image_prep_accuracy.py [--out FILE]
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
        raise SystemExit("image_prep_accuracy.py measures on a GPU; none is visible")
    import image_prep_cases as ic

    groups = {}
    for name in ic.case_names():
        case = ic.cases()[name]
        got = ic.run(case, "cuda")
        err, bar = ic.max_error(got, case), ic.bar(case)
        same = torch.equal(got.cpu().view(torch.int32), ic.run(case, "cpu").view(torch.int32))
        g = groups.setdefault(name.split("_")[0], dict(cases=0, err=0.0, ratio=0.0, worst="", bar=0.0, host_equal=True))
        g["cases"] += 1
        g["host_equal"] &= same
        if err / bar >= g["ratio"]:
            g.update(err=err, ratio=err / bar, worst=name, bar=bar)
    lines = [f"prepare_images on {torch.cuda.get_device_name(0)}: float32 CHW result against the float64 oracle, K = {ic.K_ROUNDED_OPS}"]
    for key, g in groups.items():
        lines.append(f"  {key:<10} {g['cases']:3d} cases  largest error / bar {g['ratio']:.3f} ({g['err']:.3e} of {g['bar']:.3e}, "
                     f"{g['worst']})  device == host entry bit for bit: {g['host_equal']}")
    worst = max(groups.values(), key=lambda g: g["ratio"])
    lines.append(f"  all        {sum(g['cases'] for g in groups.values()):3d} cases  largest error / bar {worst['ratio']:.3f} "
                 f"({worst['err']:.3e} of {worst['bar']:.3e}, {worst['worst']})  device == host entry bit for bit: "
                 f"{all(g['host_equal'] for g in groups.values())}")
    print("\n".join(lines), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
