#!/usr/bin/env python3
"""Time cpd_amd.kitti_eval.get_official_eval_result on synthetic KITTI-format sets (cpd_amd.synthetic.kitti_annos):
KITTI val size (3769 frames) and 40 k frames. Prints one JSON line per size: end-to-end wall time (median of --reps
calls after one warm-up) and the summed device time of the kitti_* kernels of one call (torch profiler).
Not part of bench.py. Usage: python tools/kitti_eval_time.py [--frames 3769 40000] [--reps 3]"""
import argparse
import json
import os
import re
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cpd_amd import kitti_eval  # noqa: E402
from cpd_amd.synthetic import kitti_annos  # noqa: E402

CLASSES = ["Car", "Pedestrian", "Cyclist"]


def kernel_ms(gt, dt):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        kitti_eval.get_official_eval_result(gt, dt, CLASSES)
        torch.cuda.synchronize()
    per = {}
    for e in prof.events():
        m = re.search(r"kitti_\w+_kernel", e.name)
        if m:
            t = getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0)
            per[m.group(0)] = per.get(m.group(0), 0.0) + t / 1000.0
    return per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[3769, 40000])
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    for n in args.frames:
        gt, dt = kitti_annos(n, seed=1)
        kitti_eval.get_official_eval_result(gt, dt, CLASSES)           # warm-up (module load, allocator)
        times = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            kitti_eval.get_official_eval_result(gt, dt, CLASSES)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        per = kernel_ms(gt, dt)
        print(json.dumps({"frames": n, "gt": int(sum(len(a["name"]) for a in gt)),
                          "dt": int(sum(len(a["name"]) for a in dt)), "end_to_end_s": float(np.median(times)),
                          "kernel_ms": round(sum(per.values()), 3),
                          "per_kernel_ms": {k: round(v, 3) for k, v in sorted(per.items())}}), flush=True)


if __name__ == "__main__":
    main()
