#!/usr/bin/env python3
"""Time cpd_ppscore (cpd_amd.ppscore, the PP-score precompute) at full size: one current frame against the T = 12 traversals of
the default window (max_win 30, win_inte 5) of a float16 cpd_amd.synthetic.ppscore_sequence drive at Waymo azimuth resolution
(64 x 2650 rays per sweep), poses a few kilometres from the origin.
  * gpu_ms_per_frame: steady-state device time of one call (transform, grid, counts and H; the frames are already on the
    device, file I/O excluded), from HIP events around `reps` back-to-back calls after a warm-up;
  * wall_ms_per_frame: the same calls by the host clock, ending in a synchronise (launch overhead and the device-side
    concatenation of the traversals included);
  * where scipy imports: scipy_s_per_frame, one core building a cKDTree per traversal and calling
    query_ball_point(return_length=True) on the same inputs on the same box, and whether its counts equal the GPU's;
  * bar_ms = scipy_s_per_frame / 16 in ms (sixteen ideal workers of the CPU path) and whether the GPU time is below it.
Prints one JSON line. Not part of bench.py. Usage: python tools/ppscore_time.py [--reps 20] [--n-az 2650]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cpd_amd import ppscore  # noqa: E402
from cpd_amd.synthetic import ppscore_sequence  # noqa: E402

T, CUR, RADIUS = 12, 6, 0.3     # range(i - 30, i + 30, 5): the current frame is the seventh of its twelve traversals


def scipy_counts(cur, frames, poses):
    from scipy.spatial import cKDTree
    inv = np.linalg.inv(poses[CUR])
    t0 = time.perf_counter()
    cols = []
    for f, p in zip(frames, poses):
        homo = np.ones((len(f), 4), np.float32)
        homo[:, :3] = f[:, :3]
        world = (p @ homo.T).T.astype(np.float32)      # float64 product, float32 result; column 3 stays 1
        local = (inv @ world.T).T.astype(np.float32)[:, :3]
        cols.append(cKDTree(local).query_ball_point(cur[:, :3], r=RADIUS, return_length=True))
    counts = np.stack(cols, 1)
    total = counts.sum(1, keepdims=True) + 1e-8
    prob = counts / total
    h = (-prob * np.log(prob + 1e-8)).sum(1) / np.log(len(frames))
    return counts, h, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n-az", type=int, default=2650)
    ap.add_argument("--no-scipy", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ppscore_time.py needs a GPU"
    frames, poses = ppscore_sequence(900, T, args.n_az, np.float16, origin=(5000.0, 2500.0, 0.0), frame_step=5)
    g = ppscore.PPScoreGPU()
    dev = [g.upload(f) for f in frames]
    inv = np.linalg.inv(poses[CUR])
    call = lambda: g.run(dev[CUR], dev, poses, inv, RADIUS)
    for _ in range(3):
        counts, h = call()
    torch.cuda.synchronize()
    gpu_counts, gpu_h = counts.cpu().numpy(), h.cpu().numpy()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record()
    for _ in range(args.reps):
        call()
    ev1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / args.reps
    res = {"traversals": T, "points_per_frame": int(np.mean([len(f) for f in frames])), "query_points": len(frames[CUR]),
           "ref_points": int(sum(len(f) for f in frames)), "reps": args.reps,
           "gpu_ms_per_frame": round(ev0.elapsed_time(ev1) / args.reps, 3), "wall_ms_per_frame": round(wall * 1e3, 3),
           "mean_count": round(float(gpu_counts.mean()), 2), "max_count": int(gpu_counts.max()),
           "share_h_above_0.7": round(float((gpu_h.astype(np.float64) > 0.7).mean()), 4)}
    try:
        if args.no_scipy:
            raise ImportError("skipped")
        import scipy
        c, h, sec = scipy_counts(frames[CUR], frames, poses)
        res.update({"scipy": scipy.__version__, "scipy_s_per_frame": round(sec, 3), "bar_ms": round(sec * 1e3 / 16, 3),
                    "counts_equal_scipy": bool(np.array_equal(c, gpu_counts)),
                    "h_float16_differ": int((h.astype(np.float16).view(np.uint16) != gpu_h.view(np.uint16)).sum()),
                    "below_bar": bool(res["gpu_ms_per_frame"] < sec * 1e3 / 16)})
    except ImportError as e:
        res["scipy"] = "not importable (%s)" % e
    print(json.dumps(res))


if __name__ == "__main__":
    main()
